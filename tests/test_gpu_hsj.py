"""GPU: the label-only black-box attack — the six entry points of include/advstep_hsj.h against the BYTES of their numpy float32 /
int32 restatement (tests/hsj_cpu_ops.py: every kernel is single rounded float32 operations or integers, so there is no tolerance
anywhere in the kernel tests) on every shape at which a path changes; HopSkipJump on a linear detector with dyadic data, byte for
byte against the CPU table's run; HopSkipJump on LCNN; the loop."""

import numpy as np
import pytest
import torch

from tests import hsj_cpu_ops as C
from tests.test_gpu_apgd import atk_call_context, detector, same
from tests.test_gpu_momentum import padded, untouched
from tests.test_gpu_spsa import chunks, on_side_stream

pytestmark = pytest.mark.gpu

# one sample; fewer than a quad, a quad, one more; round the 256-sample wavefront load; T % 4 != 0 (sample by sample, unaligned later
# rows: 1, 3, 5, 255, 257, 1021) and T % 4 == 0 (16-byte accesses: 4, 256, 4100); more than one 4096-sample tile (4100); one row,
# several, more rows than kinds of row; the production row
SHAPES = [(B, T) for T in (1, 3, 4, 5, 255, 256, 257, 1021, 4100) for B in (1, 3, 17)] + [(1, 64_600)]
# one probe; several in one Philox word and more (7); a whole Philox call (32), one direction into the second call (33), several (40)
DIRECTIONS = (1, 7, 32, 33, 40)
TRIALS = (1, 3)
FILL = 3.5
SEED = (0x01234567 << 32) | 0x89ABCDEF            # non-zero high words; the offset's low word carries into the high one at call 1
OFFSET = (5 << 32) | 0xFFFFFFFF
XI_REL = 0.7
KINDS = ("mixed, label 0", "mixed, label 1", "inactive", "all adversarial", "none adversarial", "one NaN logit", "dist 0")


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def batch(B, T, n, seed, K=3):
    """One batch with a row of every kind (B = 17; smaller batches take the kinds in turn, starting at T % 7): rows whose probes
    are mixed, of each label; an inactive row (copied: its -0 keeps the sign); a row whose probes are all adversarial (c = n) and
    one with none (c = 0); a row with a NaN among its logits (class 0); an active row with dist = 0.  cur has samples ON 0 and 1
    and beside them by less than, exactly and more than the row's probe and step sizes, so that both clamps act."""
    g = torch.Generator().manual_seed(seed)
    orig = torch.rand(B, T, generator=g)
    cur = torch.rand(B, T, generator=g)
    dist = torch.rand(B, generator=g) * 0.09 + 0.01
    mag = torch.rand(B, generator=g) * 0.009 + 0.001
    z = torch.randn(max(n, 1), B, generator=g)[:n]
    zc = torch.randn(K, B, generator=g)
    y = torch.randint(0, 2, (B,), generator=g)
    active = torch.ones(B, dtype=torch.int32)
    kinds = []
    for b in range(B):
        kind = KINDS[(b + T) % len(KINDS)]
        kinds.append(kind)
        m = float(mag[b])
        special = torch.tensor([0.0, 1.0, m / 2, 1.0 - m / 2, m, 1.0 - m, 2 * m, 1.0 - 2 * m, float(dist[b]) * XI_REL / 2, -0.0])
        where = torch.randint(0, T, (min(T, 24),), generator=g)
        cur[b, where] = special[torch.arange(where.numel()) % special.numel()]
        if kind.startswith("mixed"):
            y[b] = int(kind[-1])
            if n >= 2:
                z[0, b], z[1, b] = 1.0, -1.0                                                 # both decisions occur
        elif kind == "inactive":
            active[b] = 0
            cur[b, T // 2] = -0.0
        elif kind == "all adversarial":
            y[b] = 0
            z[:, b] = z[:, b].abs() + 0.125
        elif kind == "none adversarial":
            y[b] = 1
            z[:, b] = z[:, b].abs() + 0.125
        elif kind == "one NaN logit":
            y[b] = 0
            if n >= 1:
                z[b % n, b] = float("nan")
        else:
            dist[b] = 0.0
        if b % 3 == 0:                                                                       # no candidate is adversarial
            zc[:, b] = zc[:, b].abs() + 0.125 if y[b] == 1 else -zc[:, b].abs()
        elif b % 3 == 1:                                                                     # only the last one is
            zc[:, b] = zc[:, b].abs() + 0.125 if y[b] == 1 else -zc[:, b].abs()
            zc[K - 1, b] = -1.0 if y[b] == 1 else 1.0
    queries =torch.randint(1, 1000, (B,), generator=g).to(torch.int32)
    return {"orig": orig, "cur": cur, "dist": dist, "mag": mag, "z": z, "zc": zc, "y": y, "active": active, "queries": queries,
            "kinds": kinds}


def dev(d, cuda):
    return {k: (v.to(cuda) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def guarded_queries(q0, cuda):
    buf = torch.full((q0.numel() + 64,), -77, dtype=torch.int32, device=cuda)
    q = buf[32:32 + q0.numel()]
    q.copy_(q0)
    return buf, q


def guards_intact(buf, B):
    return bool((buf[:32] == -77).all() and (buf[32 + B:] == -77).all())


# ---- the probes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", SHAPES)
def test_probe_kernel_bytes(cuda, B, T):
    """Every slot equals the table's bytes (there is no copy of cur among them); inactive rows are cur's bytes; the guard round `out`
    is untouched; a fill in chunks (s0 > 0, odd ns) equals the whole one; a rerun and a run on a side stream give the same bits."""
    ops = hip()
    h = batch(B, T, 1, 31 * B + T)
    d = dev(h, cuda)
    for n in DIRECTIONS if T < 64_600 else (8,):
        want = t32(C.probe_np(h["cur"].numpy(), h["mag"].numpy(), h["active"].numpy(), SEED, OFFSET, 0, n))
        if B * T >= 255 and bool(h["active"].any()):                                        # both clamps act, and rows move
            assert float(want.min()) == 0.0 and float(want.max()) == 1.0 and bool((want[0] != h["cur"]).any())
        buf, out = padded((n, B, T), FILL, cuda)
        assert ops.hsj_probe(d["cur"], d["mag"], d["active"], SEED, OFFSET, s0=0, ns=n, out=out) is out
        torch.cuda.synchronize()
        assert untouched(buf, FILL, n * B * T)
        assert torch.equal(bits(out), bits(want)), n
        idle = h["active"] == 0
        assert torch.equal(bits(out[:, idle]), bits(h["cur"][idle].expand(n, -1, -1)))       # -0 included
        parts = []
        for s0, ns in chunks(n):
            pbuf, part = padded((ns, B, T), FILL, cuda)
            ops.hsj_probe(d["cur"], d["mag"], d["active"], SEED, OFFSET, s0=s0, ns=ns, out=part)
            torch.cuda.synchronize()
            assert untouched(pbuf, FILL, ns * B * T)
            parts.append(part)
        assert torch.equal(bits(torch.cat(parts)), bits(want)), n
        fresh = ops.hsj_probe(d["cur"], d["mag"], d["active"], SEED, OFFSET, s0=0, ns=n)
        assert fresh.shape == (n, B, T) and torch.equal(bits(fresh), bits(want))
        assert torch.equal(bits(ops.hsj_probe(d["cur"], d["mag"], d["active"], SEED, OFFSET, s0=0, ns=n)), bits(want))   # a rerun
        other = on_side_stream(cuda, lambda: ops.hsj_probe(d["cur"], d["mag"], d["active"], SEED, OFFSET, s0=0, ns=n))
        assert torch.equal(bits(other), bits(want))
    assert same(d["cur"], h["cur"])


# ---- the candidates -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", SHAPES)
def test_candidates_kernel_bytes(cuda, B, T):
    """Every slot equals the table's bytes, and for active rows clamp(cur + xi_k s) with the table's integer s; rows with dist == 0
    and inactive rows are cur; c = 0, c = n, mixed and NaN rows are all present at B = 17; at even n an all-agree row has samples
    with s = 0, which do not move; guards, a fresh output, a rerun and a side stream."""
    ops = hip()
    for n in DIRECTIONS if T < 64_600 else (8,):
        h = batch(B, T, n, 17 * B + T + n)
        d = dev(h, cuda)
        vote = C.vote_np(h["z"].numpy(), h["y"].numpy(), T, SEED, OFFSET)
        phi = np.stack([C.adversarial(h["z"].numpy()[j], h["y"].numpy()) for j in range(n)])
        for b, kind in enumerate(h["kinds"]):
            c = int(phi[:, b].sum())
            if kind == "all adversarial":
                assert c == n
            if kind == "none adversarial":
                assert c == 0
            if kind.startswith("mixed") and n >= 2:
                assert 0 < c < n
            if kind in ("all adversarial", "none adversarial") and n % 2 == 0 and T >= 255:
                assert bool((vote[b] == 0).any())                                           # a sample with s = 0
        s = t32(np.sign(vote).astype(np.float32))
        for K in TRIALS if T < 64_600 else (4,):
            want = t32(C.candidates_np(h["cur"].numpy(), h["z"].numpy(), h["y"].numpy(), h["dist"].numpy(), h["active"].numpy(),
                                       XI_REL, K, SEED, OFFSET))
            assert not torch.isnan(want).any()
            buf, out = padded((K, B, T), FILL, cuda)
            assert ops.hsj_candidates(d["cur"], d["z"], d["y"], d["dist"], d["active"], XI_REL, K, SEED, OFFSET, out=out) is out
            torch.cuda.synchronize()
            assert untouched(buf, FILL, K * B * T)
            assert torch.equal(bits(out), bits(want)), (n, K)
            act = h["active"] != 0
            xi = h["dist"] * np.float32(XI_REL)
            for k in range(K):
                eager = torch.clamp(h["cur"] + (xi * 0.5 ** k)[:, None] * s, 0, 1)
                assert torch.equal(out[k].cpu()[act], eager[act]), (n, K, k)
                assert torch.equal(bits(out[k].cpu()[~act]), bits(h["cur"][~act]))           # inactive: the bytes, -0 included
                still = act & (h["dist"] == 0)
                assert torch.equal(out[k].cpu()[still], h["cur"][still])                     # dist == 0: cur
                assert torch.equal(out[k].cpu()[act][s[act] == 0], h["cur"][act][s[act] == 0])
            fresh = ops.hsj_candidates(d["cur"], d["z"], d["y"], d["dist"], d["active"], XI_REL, K, SEED, OFFSET)
            assert fresh.shape == (K, B, T) and torch.equal(bits(fresh), bits(want))
            again = ops.hsj_candidates(d["cur"], d["z"], d["y"], d["dist"], d["active"], XI_REL, K, SEED, OFFSET)
            assert torch.equal(bits(again), bits(want))
            other = on_side_stream(cuda, lambda: ops.hsj_candidates(d["cur"], d["z"], d["y"], d["dist"], d["active"], XI_REL, K,
                                                                    SEED, OFFSET))
            assert torch.equal(bits(other), bits(want))
        assert same(d["cur"], h["cur"]) and same(d["z"], h["z"])


# ---- the choice ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", SHAPES)
def test_take_kernel_bytes(cuda, B, T):
    """out and queries equal the table's; a row takes the FIRST adversarial slot and counts n + k + 1, a row with none stays and
    counts n + K, an inactive row stays and counts nothing; in place, only the rows that move change; guards round out and queries."""
    ops = hip()
    n = 33
    for K in TRIALS:
        h = batch(B, T, n, 5 * B + T + K, K=K)
        d = dev(h, cuda)
        cand = torch.rand(K, B, T, generator=torch.Generator().manual_seed(K + T))
        cand_d = cand.to(cuda)
        want, want_q, used = C.take_np(h["cur"].numpy(), cand.numpy(), h["zc"].numpy(), h["y"].numpy(), h["active"].numpy(),
                                       h["queries"].numpy(), n)
        want, want_q, used = t32(want), t32(want_q), t32(used)
        act = h["active"] != 0
        adv = t32(np.stack([C.adversarial(h["zc"].numpy()[k], h["y"].numpy()) for k in range(K)]))
        for b in range(B):
            first = next((k for k in range(K) if adv[k, b]), None)
            src = h["cur"][b] if (first is None or not act[b]) else cand[first, b]
            assert torch.equal(bits(want[b]), bits(src))
            assert int(want_q[b] - h["queries"][b]) == (0 if not act[b] else n + (K if first is None else first + 1))

        def launch(out=None, cur_in=d["cur"]):
            qbuf, q = guarded_queries(h["queries"], cuda)
            res = ops.hsj_take(cur_in, cand_d, d["zc"], d["y"], d["active"], q, n, out=out)
            torch.cuda.synchronize()
            assert guards_intact(qbuf, B)
            return res, q

        buf, out = padded((B, T), FILL, cuda)
        res, q = launch(out)
        assert res is out and untouched(buf, FILL, B * T)
        assert torch.equal(bits(out), bits(want)) and torch.equal(q.cpu(), want_q), K
        alias_buf, alias = padded((B, T), FILL, cuda)
        alias.copy_(h["cur"])
        res, q = launch(alias, alias)
        assert res is alias and untouched(alias_buf, FILL, B * T)
        assert torch.equal(bits(alias), bits(want)) and torch.equal(q.cpu(), want_q)
        fresh, q = launch()
        assert torch.equal(bits(fresh), bits(want)) and torch.equal(q.cpu(), want_q)
        other, q = on_side_stream(cuda, launch)
        assert torch.equal(bits(other), bits(want)) and torch.equal(q.cpu(), want_q)
        assert same(d["cur"], h["cur"]) and same(cand_d, cand)


# ---- the boundary search ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T", SHAPES)
def test_search_kernels_bytes(cuda, B, T):
    """open, two rounds and close against the table, each fed the previous launch's own state: the probes, the states (inactive
    rows: every plane dist), the closed rows (hi < dist0: point(hi); else cur's bytes) and the queries; close in place and into a
    fresh output; guards round every output; a rerun of a round and a run on a side stream give the same bits."""
    ops = hip()
    h = batch(B, T, 3, 7 * B + T)
    h["dist"] = t32(C.linf_np(h["orig"].numpy(), h["cur"].numpy()))
    d = dev(h, cuda)
    cur, orig, y, active = (h[k].numpy() for k in ("cur", "orig", "y", "active"))
    zs = h["z"].clone()                                                                     # (3, B): the judgements of three probes
    zs[2, 1::4] = 0.0                                                                       # +-0 is class 0
    want_p, want_s = C.search_open_np(cur, orig, h["dist"].numpy(), active)
    pbuf, probe = padded((B, T), FILL, cuda)
    sbuf, state = padded((4, B), FILL, cuda, pad=64)
    assert ops.hsj_search_open(d["cur"], d["orig"], d["dist"], d["active"], probe, state=state) is state
    torch.cuda.synchronize()
    assert untouched(pbuf, FILL, B * T) and untouched(sbuf, FILL, 4 * B, pad=64)
    assert torch.equal(bits(probe), bits(t32(want_p))) and torch.equal(bits(state), bits(t32(want_s)))
    idle = h["active"] == 0
    assert torch.equal(bits(probe.cpu()[idle]), bits(h["cur"][idle]))
    assert torch.equal(state.cpu()[:, idle], h["dist"][idle].expand(4, -1))
    fresh_state = ops.hsj_search_open(d["cur"], d["orig"], d["dist"], d["active"], torch.empty_like(probe))
    assert torch.equal(bits(fresh_state), bits(t32(want_s)))

    for rnd in range(2):
        want_p, want_s2 = C.search_next_np(cur, orig, zs[rnd].numpy(), y, active, want_s)
        sbuf2, state2 = padded((4, B), FILL, cuda, pad=64)
        z_d = zs[rnd].to(cuda)
        assert ops.hsj_search_next(d["cur"], d["orig"], z_d, d["y"], d["active"], state, probe, state_out=state2) is state2
        torch.cuda.synchronize()
        assert untouched(pbuf, FILL, B * T) and untouched(sbuf2, FILL, 4 * B, pad=64)
        assert torch.equal(bits(probe), bits(t32(want_p))) and torch.equal(bits(state2), bits(t32(want_s2))), rnd
        assert torch.equal(bits(state), bits(t32(want_s)))                                  # the state read is left as it was
        again = torch.empty_like(probe)
        fresh = on_side_stream(cuda, lambda: ops.hsj_search_next(d["cur"], d["orig"], z_d, d["y"], d["active"], state, again))
        assert torch.equal(bits(fresh), bits(state2)) and torch.equal(bits(again), bits(probe))
        state, want_s, sbuf = state2, want_s2, sbuf2

    want, want_q = C.search_close_np(cur, orig, zs[2].numpy(), y, active, want_s, h["queries"].numpy(), 3)
    want, want_q = t32(want), t32(want_q)
    _, bhi, d0 = C._decide(zs[2].numpy(), y, want_s)
    moved = t32((active != 0) & (bhi < d0))
    assert torch.equal(bits(want[~moved]), bits(h["cur"][~moved]))                          # cur's BYTES, not point(dist0)
    assert torch.equal(want_q - h["queries"], torch.where(h["active"] != 0, 3, 0).to(torch.int32))
    z_d = zs[2].to(cuda)

    def close(out=None, cur_in=d["cur"]):
        qbuf, q = guarded_queries(h["queries"], cuda)
        res = ops.hsj_search_close(cur_in, d["orig"], z_d, d["y"], d["active"], state, q, 3, out=out)
        torch.cuda.synchronize()
        assert guards_intact(qbuf, B)
        return res, q

    buf, out = padded((B, T), FILL, cuda)
    res, q = close(out)
    assert res is out and untouched(buf, FILL, B * T)
    assert torch.equal(bits(out), bits(want)) and torch.equal(q.cpu(), want_q)
    alias_buf, alias = padded((B, T), FILL, cuda)
    alias.copy_(h["cur"])
    res, q = close(alias, alias)
    assert res is alias and untouched(alias_buf, FILL, B * T)
    assert torch.equal(bits(alias), bits(want)) and torch.equal(q.cpu(), want_q)
    fresh, q = close()
    assert torch.equal(bits(fresh), bits(want)) and torch.equal(q.cpu(), want_q)
    other, q = on_side_stream(cuda, close)
    assert torch.equal(bits(other), bits(want)) and torch.equal(q.cpu(), want_q)
    assert same(d["cur"], h["cur"]) and same(d["orig"], h["orig"])


# ---- other bounds, seeds and alignment ------------------------------------------------------------------------------------------------------

def test_other_bounds_seeds_and_unaligned_rows(cuda):
    """lo and hi other than 0 and 1 in every kernel that clamps; another seed and another offset (non-zero high words) give other
    probes and candidates, equal to the table's; T % 4 == 0 from a base one float off a 16-byte boundary takes the sample-by-sample
    path with the same bytes."""
    ops = hip()
    B, T, n, K = 3, 4100, 7, 3
    h = batch(B, T, n, 5)
    h["active"][:] = 1
    h["dist"] = t32(C.linf_np(h["orig"].numpy(), h["cur"].numpy()))
    d = dev(h, cuda)
    np_ = {k: v.numpy() for k, v in h.items() if isinstance(v, torch.Tensor)}
    shifted = torch.empty(B * T + 1, device=cuda)[1:].view(B, T)
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(h["cur"])
    for lo, hi in ((0.0, 1.0), (0.25, 0.75)):
        want = t32(C.probe_np(np_["cur"], np_["mag"], np_["active"], SEED, OFFSET, 0, n, lo, hi))
        assert torch.equal(bits(ops.hsj_probe(d["cur"], d["mag"], d["active"], SEED, OFFSET, ns=n, lo=lo, hi=hi)), bits(want))
        assert torch.equal(bits(ops.hsj_probe(shifted, d["mag"], d["active"], SEED, OFFSET, ns=n, lo=lo, hi=hi)), bits(want))
        want = t32(C.candidates_np(np_["cur"], np_["z"], np_["y"], np_["dist"], np_["active"], XI_REL, K, SEED, OFFSET, lo, hi))
        for c in (d["cur"], shifted):
            got = ops.hsj_candidates(c, d["z"], d["y"], d["dist"], d["active"], XI_REL, K, SEED, OFFSET, lo=lo, hi=hi)
            assert torch.equal(bits(got), bits(want))
        want_p, want_s = C.search_open_np(np_["cur"], np_["orig"], np_["dist"], np_["active"], lo, hi)
        for c in (d["cur"], shifted):
            probe = torch.empty(B, T, device=cuda)
            state = ops.hsj_search_open(c, d["orig"], d["dist"], d["active"], probe, lo=lo, hi=hi)
            assert torch.equal(bits(probe), bits(t32(want_p))) and torch.equal(bits(state), bits(t32(want_s)))
        z = torch.tensor([1.0, -1.0, 1.0])
        want_p, want_s2 = C.search_next_np(np_["cur"], np_["orig"], z.numpy(), np_["y"], np_["active"], want_s, lo, hi)
        want_c, _ = C.search_close_np(np_["cur"], np_["orig"], z.numpy(), np_["y"], np_["active"], want_s, np_["queries"], 1, lo, hi)
        for c in (d["cur"], shifted):
            probe = torch.empty(B, T, device=cuda)
            state2 = ops.hsj_search_next(c, d["orig"], z.to(cuda), d["y"], d["active"], state, probe, lo=lo, hi=hi)
            assert torch.equal(bits(probe), bits(t32(want_p))) and torch.equal(bits(state2), bits(t32(want_s2)))
            got = ops.hsj_search_close(c, d["orig"], z.to(cuda), d["y"], d["active"], state, d["queries"].clone(), 1, lo=lo, hi=hi)
            assert torch.equal(bits(got), bits(t32(want_c)))
        cand = ops.hsj_candidates(d["cur"], d["z"], d["y"], d["dist"], d["active"], XI_REL, K, SEED, OFFSET)
        took = ops.hsj_take(shifted, cand, d["zc"], d["y"], d["active"], d["queries"].clone(), n)
        assert torch.equal(bits(took), bits(ops.hsj_take(d["cur"], cand, d["zc"], d["y"], d["active"], d["queries"].clone(), n)))
    base_p = ops.hsj_probe(d["cur"], d["mag"], d["active"], SEED, OFFSET, ns=n)
    base_c = ops.hsj_candidates(d["cur"], d["z"], d["y"], d["dist"], d["active"], XI_REL, K, SEED, OFFSET)
    for seed, offset in ((SEED + 1, OFFSET), (SEED ^ (1 << 50), OFFSET), (SEED, OFFSET + 1), (SEED, OFFSET ^ (1 << 40))):
        other = ops.hsj_probe(d["cur"], d["mag"], d["active"], seed, offset, ns=n)
        assert not torch.equal(other, base_p)
        assert torch.equal(bits(other), bits(t32(C.probe_np(np_["cur"], np_["mag"], np_["active"], seed, offset, 0, n))))
        other = ops.hsj_candidates(d["cur"], d["z"], d["y"], d["dist"], d["active"], XI_REL, K, seed, offset)
        assert not torch.equal(other, base_c)
        assert torch.equal(bits(other), bits(t32(C.candidates_np(np_["cur"], np_["z"], np_["y"], np_["dist"], np_["active"], XI_REL,
                                                                 K, seed, offset))))


def test_wrappers_refuse_bad_arguments(cuda):
    ops = hip()
    x = torch.zeros(3, 8, device=cuda)
    f = torch.zeros(3, device=cuda)
    y = torch.zeros(3, dtype=torch.int64, device=cuda)
    a = torch.ones(3, dtype=torch.int32, device=cuda)
    q = torch.zeros(3, dtype=torch.int32, device=cuda)
    st = torch.zeros(4, 3, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        ops.hsj_probe(x.double(), f, a, 1)
    with pytest.raises(TypeError, match="int32"):
        ops.hsj_probe(x, f, a.long(), 1)
    with pytest.raises(ValueError, match="slots"):
        ops.hsj_probe(x, f, a, 1, s0=-1)
    with pytest.raises(ValueError, match="slots"):
        ops.hsj_probe(x, f, a, 1, s0=1, ns=C.MAX_DIRECTIONS)
    with pytest.raises(ValueError, match="out must hold"):
        ops.hsj_probe(x, f, a, 1, ns=2, out=torch.zeros(3, 3, 8, device=cuda))
    with pytest.raises(ValueError, match="contiguous"):
        ops.hsj_probe(x.t(), f, a, 1)
    with pytest.raises(ValueError, match="one value per row"):
        ops.hsj_probe(x, f[:2], a, 1)
    with pytest.raises(ValueError, match=r"z must be \(n, 3\)"):
        ops.hsj_candidates(x, torch.zeros(5, 2, device=cuda), y, f, a, 0.5, 2, 1)
    with pytest.raises(ValueError, match="at most 1024"):
        ops.hsj_candidates(x, torch.zeros(1025, 3, device=cuda), y, f, a, 0.5, 2, 1)
    with pytest.raises(ValueError, match="trials"):
        ops.hsj_candidates(x, torch.zeros(5, 3, device=cuda), y, f, a, 0.5, 9, 1)
    with pytest.raises(ValueError, match="cand must hold"):
        ops.hsj_take(x, torch.zeros(3, 3, 8, device=cuda), torch.zeros(2, 3, device=cuda), y, a, q, 5)
    with pytest.raises(ValueError, match=r"state must be \(4, 3\)"):
        ops.hsj_search_next(x, x.clone(), f, y, a, st[:3], x.clone())
    with pytest.raises(ValueError, match="does not match"):
        ops.hsj_search_open(x, x[:2].clone(), f, a, x.clone())
    with pytest.raises(ValueError, match="rounds"):
        ops.hsj_search_close(x, x.clone(), f, y, a, st, q, -1)
    from audio_deepfake_adversarial_attacks_amd import _lib
    with pytest.raises(_lib.AdvstepError):
        ops.hsj_search_next(x, x.clone(), f, y, a, st, x.clone(), state_out=st)             # in place: not a ping-pong
    with pytest.raises(_lib.AdvstepError):
        ops.hsj_search_open(x, x.clone(), f, a, x)                                          # out is cur
    empty = torch.zeros(0, 8, device=cuda)
    e1, e32 = torch.zeros(0, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda)
    assert ops.hsj_probe(empty, e1, e32, 1, ns=3).shape == (3, 0, 8)                        # B = 0: nothing launched


# ---- end to end: exact on a linear detector ---------------------------------------------------------------------------------------------

def hsj(model, ops=None, **kw):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    atk = torchattacks.HopSkipJump(model, **kw)
    if ops is not None:
        atk.ops = ops
    return atk


@pytest.fixture(scope="module")
def table_run():
    """The attack through the CPU table on C.dyadic_case, computed once: (model, x, y, adv, radius, queries)."""
    model, x, y = C.dyadic_case()
    table = hsj(model, C, **C.DYADIC)
    torch.manual_seed(11)
    want = table(x, y)
    return model, x, y, want, table.last_radius.clone(), table.last_queries.clone(), table.budget


@pytest.mark.parametrize("max_rows", [1024, 20])
def test_attack_on_a_linear_detector_equals_the_cpu_table(cuda, table_run, max_rows):
    """C.dyadic_case: every forwarded sample lies on the grid 2^-24 (asserted inside the model on both sides) and every logit is
    exact in any order of summation, so the attack on the device must return the bytes, the radii and the queries of the attack
    through the CPU table.  The table's own run has the row that is wrong from the start, rows that freeze below eps before the
    end and rows that never do (asserted), and every row starts from a donor, so no noise is drawn."""
    model, x, y, want, radius, q, budget = table_run
    assert q[0] == 1 and radius[0] == 0 and bool(torch.isfinite(radius).all())
    assert bool((q[1:] < q.max()).any()) and bool((radius > C.DYADIC["eps"]).any()) and bool((radius[1:] <= C.DYADIC["eps"]).any())
    inner = model.inner
    gpu_model = C.GridChecked(C.LinearDetector(inner.w.detach().float(), inner.bias).to(cuda))
    atk = hsj(gpu_model, max_rows=max_rows, **C.DYADIC)
    torch.manual_seed(11)
    got = atk(x.to(cuda), y.to(cuda))
    assert got.is_cuda and atk.last_queries.is_cuda and atk.last_queries.dtype == torch.int32
    assert atk.last_radius.is_cuda and atk.last_radius.dtype == torch.float32 and gpu_model.rows > 0
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(atk.last_radius), bits(radius))
    assert torch.equal(atk.last_queries.cpu(), q)


# ---- end to end: on the detector -------------------------------------------------------------------------------------------------------

DETECTOR_SEED = 47


def test_attack_on_lcnn(cuda):
    """B = 2, steps = 2, init_evals = 2, search_steps = 3, step_trials = 2.  A row returned within eps is within it:
    |adv - x| <= eps (1 + 2u) + u, the float32 allowance of the PGD tests (the radius compared with eps is the float32 maximum of
    fl(adv - x), within u of the true distance); adv in [0, 1]; queries <= budget (+ init_trials for a row that starts from noise);
    the same seed gives the same bytes; no host read inside the call."""
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    model = detector("lcnn", cuda)
    x, _ = synthetic_waveforms(2, seed=DETECTOR_SEED)
    x01, _, _ = hip().to_minmax(x.to(cuda))
    with torch.no_grad():
        y = (model(x01).reshape(-1) > 0).long()                                 # both rows start classified correctly
    eps = 0.001
    kw = {"eps": eps, "steps": 2, "init_evals": 2, "search_steps": 3, "step_trials": 2}
    atk = hsj(model, **kw)
    atk.set_training_mode(model_training=True, batchnorm_training=False)

    def check(adv, a):
        u = 2.0 ** -24
        d = (adv.double() - x01.double()).abs().amax(dim=1)
        radius, queries = a.last_radius, a.last_queries
        print(f"  max |adv - x| = {d.tolist()}, eps = {eps}, radius = {radius.tolist()}, queries = {queries.tolist()}, "
              f"budget = {a.budget}")
        assert bool((d <= float(np.float32(eps)) * (1 + 2 * u) + u).all())
        assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
        assert queries.dtype == torch.int32 and queries.shape == (2,) and radius.dtype == torch.float32 and radius.shape == (2,)
        assert bool((queries >= 1).all()) and bool((queries <= a.budget + a.init_trials).all())
        assert bool((radius >= 0).all())
        moved = d > 0
        assert bool((radius[moved] <= eps).all())                               # only rows within eps come back moved

    assert atk.budget == 1 + 3 * 3 + (2 + 2) + (2 + 2)
    torch.manual_seed(3)
    first = atk(x01, y)
    q_first, r_first = atk.last_queries.clone(), atk.last_radius.clone()
    check(first, atk)
    torch.manual_seed(3)
    again = atk(x01, y)
    assert torch.equal(bits(again), bits(first)) and torch.equal(atk.last_queries, q_first)
    assert torch.equal(bits(atk.last_radius), bits(r_first))

    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).item()                                   # the mode works on this build
        torch.manual_seed(3)
        with atk_call_context(atk):
            quiet = atk.forward(x01, y)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(bits(quiet), bits(first))

    free = hsj(model, **{**kw, "eps": None})                                    # no radius to reach: whatever was found comes back
    free.set_training_mode(model_training=True, batchnorm_training=False)
    torch.manual_seed(3)
    adv = free(x01, y)
    started = torch.isfinite(free.last_radius)
    assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0 and bool((free.last_queries <= free.budget + 8).all())
    assert torch.equal(free.last_radius[started], (adv - x01).abs().amax(dim=1)[started])
    assert torch.equal(adv[~started], x01[~started])


# ---- through the loop --------------------------------------------------------------------------------------------------------------------

CFG = {"data": {"seed": 42}, "checkpoint": {"path": ""},
       "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
QUERY_KEYS = ["blackbox/queries_mean", "blackbox/queries_median", "blackbox/stopped_early", "blackbox/budget"]


def test_loop_reports_the_radii_and_the_queries(cuda):
    """generate_attacks over 8 synthetic utterances, batch 4, with the registry's class at a small budget: the min_radius/* and
    blackbox/* keys and the per-utterance radii and counts, through the loop's existing `last_radius` / `last_queries` hooks.  How
    many utterances flip is not asserted."""
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    from audio_deepfake_adversarial_attacks_amd.metrics import radius_summary
    method, params = AttackEnum["HSJ"].value
    params = {**params, "steps": 2, "init_evals": 2, "search_steps": 3, "step_trials": 2, "init_trials": 2}
    budget = 1 + 3 * 3 + 4 + 4
    torch.manual_seed(5)
    rep = generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=method, attack_params=params,
                           batch_size=4, dataset=SyntheticDetectionDataset(8), share_weights=True, shuffle=False, num_workers=0,
                           return_scores=True)
    torch.cuda.synchronize()
    assert [k for k in rep if k.startswith("blackbox/")] == QUERY_KEYS and rep["blackbox/budget"] == budget
    q = rep["scores"]["queries"]
    assert q.dtype == np.int32 and q.shape == (8,) and rep["num_total"] == 8
    assert (q >= 1).all() and (q <= budget + 2).all()
    assert rep["blackbox/queries_mean"] == float(q.mean()) and rep["blackbox/queries_median"] == float(np.median(q))
    r = rep["scores"]["min_radius"]
    assert r.dtype == np.float32 and r.shape == (8,) and (r >= 0).all() and not np.isnan(r).any()
    assert (r[np.isfinite(r)] <= 1.0).all()
    want = radius_summary(r, params["report_at"])
    keys = [k for k in rep if k.startswith("min_radius/")]
    assert keys == list(want) and len(keys) > len(params["report_at"])
    for k in keys:
        assert rep[k] == want[k] or (np.isnan(rep[k]) and np.isnan(want[k])), k
    assert 0.0 <= rep["adv_eval/accuracy"] <= 100.0
