"""GPU: the score-based black-box attack — spsa_probe and spsa_step against the BYTES of their numpy float32 restatement
(tests/spsa_cpu_ops.py: both kernels are exact-order float32 computations, so there is no tolerance anywhere in the kernel tests) on
every shape at which a path changes; the step against hip_ops.pgd_linf_step on the table's gradient; SPSA on a linear detector
with dyadic data, byte for byte against the CPU table's run; SPSA on LCNN; the loop."""

import numpy as np
import pytest
import torch

from tests import spsa_cpu_ops as C
from tests.test_gpu_apgd import atk_call_context, detector, same
from tests.test_gpu_momentum import padded, untouched

pytestmark = pytest.mark.gpu

# one sample; fewer than a quad, a quad, one more; round the 256-sample wavefront load; T % 4 != 0 (sample by sample, unaligned later
# rows: 1, 3, 5, 255, 257, 1021) and T % 4 == 0 (16-byte accesses: 4, 256, 4100); more than one 4096-sample tile (4100); one row,
# several, more rows than kinds of row; the production row
SHAPES = [(B, T) for T in (1, 3, 4, 5, 255, 256, 257, 1021, 4100) for B in (1, 3, 17)] + [(1, 64_600)]
# one pair; several; a whole Philox call (32), one direction into the second call (33), several into it (40)
DIRECTIONS = (1, 7, 32, 33, 40)
FILL = 3.5
SEED = (0x01234567 << 32) | 0x89ABCDEF            # non-zero high words; the offset's low word carries into the high one at call 1
OFFSET = (5 << 32) | 0xFFFFFFFF
DELTA, EPS, ALPHA = 0.004, 0.01, 0.003


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def on_side_stream(cuda, fn):
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        res = fn()
    side.synchronize()
    return res


def chunks(S):
    """(s0, ns) covering 0 .. S - 1 with odd sizes 1, 3, 5, 1, ... (s0 > 0 after the first; a rest of any size)."""
    out, s0, k = [], 0, 0
    while s0 < S:
        ns = min((1, 3, 5)[k % 3], S - s0)
        out.append((s0, ns))
        s0, k = s0 + ns, k + 1
    return out


# ---- the probe slots ----------------------------------------------------------------------------------------------------------------

def probe_input(B, T, seed):
    """adv in [0, 1] with samples ON lo and hi and beside them by less than, exactly and more than delta: the clamp acts."""
    g = torch.Generator().manual_seed(seed)
    adv = torch.rand(B, T, generator=g)
    special = torch.tensor([0.0, 1.0, DELTA / 2, 1.0 - DELTA / 2, DELTA, 1.0 - DELTA, 2 * DELTA, 1.0 - 2 * DELTA, -0.0])
    where = torch.randint(0, B * T, (min(B * T, 64),), generator=g)
    adv.view(-1)[where] = special[torch.arange(where.numel()) % special.numel()]
    return adv


@pytest.mark.parametrize("B,T", SHAPES)
def test_probe_kernel_bytes(cuda, B, T):
    """Every slot equals the table's bytes; the guard round `out` is untouched; a fill in chunks (s0 > 0, odd ns) equals the whole
    one; a rerun and a run on a side stream give the same bits."""
    ops = hip()
    adv = probe_input(B, T, 31 * B + T)
    adv_d = adv.to(cuda)
    for n in DIRECTIONS if T < 64_600 else (8,):
        S = 1 + 2 * n
        want = torch.from_numpy(C.spsa_probe_np(adv.numpy(), DELTA, SEED, OFFSET, 0, S))
        if B * T >= 255:                                                            # both clamps act
            assert float(want.min()) == 0.0 and float(want.max()) == 1.0 and bool((want[1:] != adv).any())
        buf, out = padded((S, B, T), FILL, cuda)
        assert ops.spsa_probe(adv_d, DELTA, SEED, OFFSET, s0=0, ns=S, out=out) is out
        torch.cuda.synchronize()
        assert untouched(buf, FILL, S * B * T)
        assert torch.equal(bits(out), bits(want)), n
        assert torch.equal(bits(out[0]), bits(adv))                                # slot 0: adv's bytes, -0 included
        parts = []
        for s0, ns in chunks(S):
            pbuf, part = padded((ns, B, T), FILL, cuda)
            ops.spsa_probe(adv_d, DELTA, SEED, OFFSET, s0=s0, ns=ns, out=part)
            torch.cuda.synchronize()
            assert untouched(pbuf, FILL, ns * B * T)
            parts.append(part)
        assert torch.equal(bits(torch.cat(parts)), bits(want)), n
        fresh = ops.spsa_probe(adv_d, DELTA, SEED, OFFSET, s0=0, ns=S)
        assert fresh.shape == (S, B, T) and torch.equal(bits(fresh), bits(want))
        other = on_side_stream(cuda, lambda: ops.spsa_probe(adv_d, DELTA, SEED, OFFSET, s0=0, ns=S))
        assert torch.equal(bits(other), bits(want))
    assert same(adv_d, adv)


def test_probe_other_bounds_seeds_and_unaligned_rows(cuda):
    """lo and hi other than 0 and 1; another seed and another offset give other slots; T % 4 == 0 from a base one float off a
    16-byte boundary takes the sample-by-sample path with the same bytes."""
    ops = hip()
    B, T, n = 3, 4100, 3
    S = 1 + 2 * n
    adv = probe_input(B, T, 5)
    adv_d = adv.to(cuda)
    got = ops.spsa_probe(adv_d, DELTA, SEED, OFFSET, ns=S, lo=0.25, hi=0.75)
    assert torch.equal(bits(got), bits(torch.from_numpy(C.spsa_probe_np(adv.numpy(), DELTA, SEED, OFFSET, 0, S, 0.25, 0.75))))
    base = ops.spsa_probe(adv_d, DELTA, SEED, OFFSET, ns=S)
    for seed, offset in ((SEED + 1, OFFSET), (SEED ^ (1 << 50), OFFSET), (SEED, OFFSET + 1), (SEED, OFFSET ^ (1 << 40))):
        other = ops.spsa_probe(adv_d, DELTA, seed, offset, ns=S)
        assert torch.equal(other[0], base[0]) and not torch.equal(other[1:], base[1:])
        assert torch.equal(bits(other), bits(torch.from_numpy(C.spsa_probe_np(adv.numpy(), DELTA, seed, offset, 0, S))))
    shifted = torch.empty(B * T + 1, device=cuda)[1:].view(B, T)
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(adv)
    assert torch.equal(bits(ops.spsa_probe(shifted, DELTA, SEED, OFFSET, ns=S)), bits(base))


def test_wrappers_refuse_bad_arguments(cuda):
    ops = hip()
    x = torch.zeros(3, 8, device=cuda)
    z = torch.zeros(5, 3, device=cuda)
    y = torch.zeros(3, dtype=torch.int64, device=cuda)
    q = torch.zeros(3, dtype=torch.int32, device=cuda)
    with pytest.raises(TypeError, match="float32"):
        ops.spsa_probe(x.double(), 0.1, 1)
    with pytest.raises(ValueError, match="slots"):
        ops.spsa_probe(x, 0.1, 1, s0=-1)
    with pytest.raises(ValueError, match="slots"):
        ops.spsa_probe(x, 0.1, 1, s0=0, ns=2 * C.MAX_DIRECTIONS + 2)
    with pytest.raises(ValueError, match="out must hold"):
        ops.spsa_probe(x, 0.1, 1, ns=2, out=torch.zeros(3, 3, 8, device=cuda))
    with pytest.raises(ValueError, match="contiguous"):
        ops.spsa_probe(x.t(), 0.1, 1)
    with pytest.raises(ValueError, match=r"z must be \(1 \+ 2n, 3\)"):
        ops.spsa_step(x, x.clone(), torch.zeros(4, 3, device=cuda), y, q, 0.1, 0.1, 1)
    with pytest.raises(ValueError, match=r"z must be \(1 \+ 2n, 3\)"):
        ops.spsa_step(x, x.clone(), torch.zeros(5, 2, device=cuda), y, q, 0.1, 0.1, 1)
    with pytest.raises(TypeError, match="int64"):
        ops.spsa_step(x, x.clone(), z, y.int(), q, 0.1, 0.1, 1)
    with pytest.raises(TypeError, match="int32"):
        ops.spsa_step(x, x.clone(), z, y, q.long(), 0.1, 0.1, 1)
    with pytest.raises(ValueError, match="one value per row"):
        ops.spsa_step(x, x.clone(), z, y[:2], q, 0.1, 0.1, 1)
    with pytest.raises(ValueError, match="does not match"):
        ops.spsa_step(x, x[:2].clone(), z, y, q, 0.1, 0.1, 1)
    assert ops.spsa_probe(torch.zeros(0, 8, device=cuda), 0.1, 1, ns=3).shape == (3, 0, 8)          # B = 0: nothing launched


# ---- the step -------------------------------------------------------------------------------------------------------------------------

KINDS = ("ordinary 0", "ordinary 1", "fooled 0", "fooled 1", "z0 == 0, label 0", "z0 == 0, label 1", "all pairs tie", "one NaN logit",
         "z0 NaN, label 1")


def step_inputs(B, T, n, seed):
    """One batch with a row of every kind (B = 17; smaller batches take the kinds in turn, starting at T % 9).  Row kinds:
    ordinary rows of each label; a fooled row of each label; z[0] == 0 with each label (class 1 is z > 0, so 0 is class 0: label
    0 is NOT fooled and moves, label 1 is fooled); a row whose pairs all tie (g = +-0: no move, but projected and counted); a row
    with one NaN logit in a pair (sign(NaN) = 0 wherever the NaN reaches, which is every sample); a NaN z[0] with label 1 (class
    0: fooled)."""
    g = torch.Generator().manual_seed(seed)
    orig = torch.rand(B, T, generator=g)
    orig.view(-1)[::13] = 0.0
    orig.view(-1)[5::17] = 1.0
    adv = torch.clamp(orig + (torch.rand(B, T, generator=g) * 2 - 1) * EPS, 0, 1)
    face = torch.rand(B, T, generator=g) < 0.2
    adv[face] = torch.clamp(orig + EPS * torch.sign(torch.rand(B, T, generator=g) - 0.5), 0, 1)[face]       # on the ball's faces
    adv.view(-1)[3::29] = -0.0                                                  # a fooled row's copy must keep the sign bit
    S = 1 + 2 * n
    z = torch.randn(S, B, generator=g)
    y = torch.zeros(B, dtype=torch.int64)
    kinds = []
    for b in range(B):
        kind = KINDS[(b + T) % len(KINDS)]
        kinds.append(kind)
        mag = float(z[0, b].abs()) + 0.125
        if kind.startswith("ordinary") or kind in ("all pairs tie", "one NaN logit"):
            y[b] = b % 2 if not kind.startswith("ordinary") else int(kind[-1])
            z[0, b] = mag if y[b] == 1 else -mag
        elif kind.startswith("fooled"):
            y[b] = int(kind[-1])
            z[0, b] = -mag if y[b] == 1 else mag
        elif kind.startswith("z0 == 0"):
            y[b] = int(kind[-1])
            z[0, b] = 0.0 if b % 2 else -0.0
        else:
            y[b] = 1
            z[0, b] = float("nan")
        if kind == "all pairs tie":
            z[2::2, b] = z[1::2, b]
        if kind == "one NaN logit":
            z[1 + 2 * (b % n) + (b // n) % 2, b] = float("nan")
    queries = torch.randint(1, 1000, (B,), generator=g).to(torch.int32)
    return adv, orig, z, y, queries, kinds


@pytest.mark.parametrize("B,T", SHAPES)
def test_step_kernel_bytes(cuda, B, T):
    """out and queries equal the table's bytes; fooled rows are adv's bytes and keep their count, active rows count S; the
    active rows equal hip_ops.pgd_linf_step on the table's g, byte for byte; out = adv in place gives the same; the guards round
    out and queries are untouched; a rerun and a run on a side stream give the same bits."""
    ops = hip()
    for n in DIRECTIONS if T < 64_600 else (8,):
        S = 1 + 2 * n
        adv, orig, z, y, q0, kinds = step_inputs(B, T, n, 17 * B + T + n)
        fooled = torch.from_numpy(C.fooled_rows(z[0].numpy(), y.numpy()))
        for b, kind in enumerate(kinds):
            assert bool(fooled[b]) == (kind.startswith("fooled") or kind in ("z0 == 0, label 1", "z0 NaN, label 1")), kind
        want, want_q = C.spsa_step_np(adv.numpy(), orig.numpy(), z.numpy(), y.numpy(), q0.numpy(), ALPHA, EPS, SEED, OFFSET)
        want, want_q = torch.from_numpy(want), torch.from_numpy(want_q)
        assert not torch.isnan(want).any()
        assert torch.equal(want_q, q0 + torch.where(fooled, 0, S).to(torch.int32))
        adv_d, orig_d, z_d, y_d = adv.to(cuda), orig.to(cuda), z.to(cuda), y.to(cuda)

        def launch(out=None, adv_in=adv_d):
            qbuf = torch.full((B + 64,), -77, dtype=torch.int32, device=cuda)
            q = qbuf[32:32 + B]
            q.copy_(q0)
            res = ops.spsa_step(adv_in, orig_d, z_d, y_d, q, ALPHA, EPS, SEED, OFFSET, out=out)
            torch.cuda.synchronize()
            assert bool((qbuf[:32] == -77).all() and (qbuf[32 + B:] == -77).all())
            return res, q

        buf, out = padded((B, T), FILL, cuda)
        res, q = launch(out)
        assert res is out and untouched(buf, FILL, B * T)
        assert torch.equal(bits(out), bits(want)), n
        assert torch.equal(q.cpu(), want_q), n
        assert torch.equal(bits(out[fooled]), bits(adv[fooled]))
        assert same(adv_d, adv) and same(orig_d, orig) and same(z_d, z)

        active = ~fooled
        if active.any():
            g_table = torch.from_numpy(C.spsa_gradient_np(z.numpy(), y.numpy(), T, SEED, OFFSET))
            stepped = ops.pgd_linf_step(adv_d, g_table.to(cuda), orig_d, ALPHA, EPS)
            assert torch.equal(bits(out[active]), bits(stepped[active])), n
            for b, kind in enumerate(kinds):
                if kind == "all pairs tie":
                    assert not bool(g_table[b].any())                           # +-0 everywhere: the row takes no step
                    assert torch.equal(bits(out[b]), bits(ops.pgd_linf_step(adv_d[b:b + 1], torch.zeros(1, T, device=cuda),
                                                                            orig_d[b:b + 1], ALPHA, EPS)[0]))
                if kind == "one NaN logit":
                    assert bool(torch.isnan(g_table[b]).all())

        alias_buf, alias = padded((B, T), FILL, cuda)
        alias.copy_(adv)
        res, q = launch(alias, alias)
        assert res is alias and untouched(alias_buf, FILL, B * T)
        assert torch.equal(bits(alias), bits(want)) and torch.equal(q.cpu(), want_q)
        fresh, q = launch()
        assert torch.equal(bits(fresh), bits(want)) and torch.equal(q.cpu(), want_q)
        other, q = on_side_stream(cuda, launch)
        assert torch.equal(bits(other), bits(want)) and torch.equal(q.cpu(), want_q)


def test_step_from_unaligned_rows_and_other_bounds(cuda):
    ops = hip()
    B, T, n = 9, 4100, 7
    adv, orig, z, y, q0, _ = step_inputs(B, T, n, 3)
    for lo, hi in ((0.0, 1.0), (0.25, 0.75)):
        want, want_q = C.spsa_step_np(adv.numpy(), orig.numpy(), z.numpy(), y.numpy(), q0.numpy(), ALPHA, EPS, SEED, OFFSET, lo, hi)
        shifted = torch.empty(B * T + 1, device=cuda)[1:].view(B, T)
        assert shifted.data_ptr() % 16 == 4
        shifted.copy_(adv)
        q = q0.to(cuda)
        out = ops.spsa_step(shifted, orig.to(cuda), z.to(cuda), y.to(cuda), q, ALPHA, EPS, SEED, OFFSET, lo=lo, hi=hi)
        assert torch.equal(bits(out), bits(torch.from_numpy(want))) and torch.equal(q.cpu(), torch.from_numpy(want_q))


# ---- end to end: exact on a linear detector ---------------------------------------------------------------------------------------------

def spsa(model, ops=None, **kw):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    atk = torchattacks.SPSA(model, **kw)
    if ops is not None:
        atk.ops = ops
    return atk


@pytest.mark.parametrize("max_rows", [1024, 20])
def test_attack_on_a_linear_detector_equals_the_cpu_table(cuda, max_rows):
    """C.dyadic_case: every logit and every step is exact on both sides, so the attack on the device must return the bytes and
    the queries of the attack through the CPU table.  The table's own run has a row that is fooled before the last iteration, a
    row that never is and the row that is wrong from the start (asserted), so both branches of the step kernel decide the result."""
    model, x, y = C.dyadic_case()
    table = spsa(model, C, **C.DYADIC)
    torch.manual_seed(11)
    want = table(x, y)
    q = table.last_queries
    assert q[0] == 0 and bool(((q > 0) & (q < table.budget)).any()) and bool((q == table.budget).any())
    gpu_model = C.LinearDetector(model.w.detach().float(), model.bias).to(cuda)
    atk = spsa(gpu_model, max_rows=max_rows, **C.DYADIC)
    torch.manual_seed(11)
    got = atk(x.to(cuda), y.to(cuda))
    assert got.is_cuda and atk.last_queries.is_cuda and atk.last_queries.dtype == torch.int32
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(atk.last_queries.cpu(), q)


# ---- end to end: on the detector -------------------------------------------------------------------------------------------------------

DETECTOR_SEED = 47


def detector_batch(cuda, model):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    x, _ = synthetic_waveforms(2, seed=DETECTOR_SEED)
    x01, _, _ = hip().to_minmax(x.to(cuda))
    with torch.no_grad():
        y = (model(x01).reshape(-1) > 0).long()                                 # both rows start classified correctly
    return x01, y


def test_attack_on_lcnn(cuda):
    """B = 2, nb_sample = 2 (S = 5), steps = 3.  |adv - x| <= eps (1 + 2u) + u: the step's d = clamp(a - x, -eps, eps) is within
    the float32 eps, and adv = fl(x + d) rounds once at magnitude <= 1 (the allowance of the PGD tests); adv in [0, 1];
    last_queries a multiple of S and at most steps * S; the same seed gives the same bytes; no host read inside the call.

    Forward chunkings: LCNN's no_grad forward is bit-stable across batch sizes at these shapes (10 rows at once against pieces of
    4, 4 and 2 rows and against single rows give equal logits on the MI355X, in eval mode and in the attack's train mode with
    frozen BatchNorm; asserted below on the clean batch's first slots), so max_rows = 4 (S * B = 10 rows in pieces of 4, 4, 2)
    must return the bytes and the queries of the single forward."""
    model = detector("lcnn", cuda)
    x01, y = detector_batch(cuda, model)
    eps, S, steps = 0.001, 5, 3
    atk = spsa(model, eps=eps, steps=steps, nb_sample=2)
    atk.set_training_mode(model_training=True, batchnorm_training=False)

    def check(adv, queries):
        u = 2.0 ** -24
        d = (adv.double() - x01.double()).abs().max().item()
        print(f"  max |adv - x| = {d:.9g}, eps = {eps}, queries = {queries.tolist()}")
        assert d <= float(np.float32(eps)) * (1 + 2 * u) + u
        assert float(adv.min()) >= 0.0 and float(adv.max()) <= 1.0
        assert queries.dtype == torch.int32 and queries.shape == (2,)
        assert bool((queries % S == 0).all()) and bool((queries <= steps * S).all()) and bool((queries >= 0).all())

    torch.manual_seed(3)
    first = atk(x01, y)
    q_first = atk.last_queries.clone()
    check(first, q_first)
    assert not torch.equal(first, x01)
    torch.manual_seed(3)
    again = atk(x01, y)
    assert torch.equal(bits(again), bits(first)) and torch.equal(atk.last_queries, q_first)

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

    rows = hip().spsa_probe(x01, eps, 9, ns=S).reshape(S * 2, -1)               # what an iteration forwards
    with atk_call_context(atk), torch.no_grad():
        pieces = torch.cat([model(rows[a:a + 4]) for a in (0, 4, 8)])
        assert torch.equal(bits(model(rows)), bits(pieces))                     # the premise of the byte comparison below
    small = spsa(model, eps=eps, steps=steps, nb_sample=2, max_rows=4)          # two slots per forward, S * B = 10 rows in all
    small.set_training_mode(model_training=True, batchnorm_training=False)
    torch.manual_seed(3)
    chunked = small(x01, y)
    check(chunked, small.last_queries)
    assert torch.equal(bits(chunked), bits(first)) and torch.equal(small.last_queries, q_first)

    full = spsa(model, eps=eps, steps=steps, nb_sample=2, early_stop=False)
    full.set_training_mode(model_training=True, batchnorm_training=False)
    torch.manual_seed(3)
    check(full(x01, y), full.last_queries)
    assert full.last_queries.tolist() == [steps * S] * 2


# ---- through the loop --------------------------------------------------------------------------------------------------------------------

CFG = {"data": {"seed": 42}, "checkpoint": {"path": ""},
       "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
KEYS = ["blackbox/queries_mean", "blackbox/queries_median", "blackbox/stopped_early", "blackbox/budget"]


def test_loop_reports_the_queries(cuda):
    """generate_attacks over 8 synthetic utterances, batch 4, with the registry's class at a small budget (steps = 2, nb_sample = 2:
    S = 5): the blackbox/* keys and the per-utterance counts; the registry member itself constructs in the loop's way.  How
    many utterances flip is not asserted."""
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    method, params = AttackEnum["SPSA"].value
    params = {**params, "steps": 2, "nb_sample": 2}
    torch.manual_seed(5)
    rep = generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=method, attack_params=params,
                           batch_size=4, dataset=SyntheticDetectionDataset(8), share_weights=True, shuffle=False, num_workers=0,
                           return_scores=True)
    torch.cuda.synchronize()
    assert [k for k in rep if k.startswith("blackbox/")] == KEYS
    q = rep["scores"]["queries"]
    assert q.dtype == np.int32 and q.shape == (8,) and rep["num_total"] == 8
    assert (q % 5 == 0).all() and (q >= 0).all() and (q <= 10).all() and rep["blackbox/budget"] == 10
    assert rep["blackbox/queries_mean"] == float(q.mean()) and rep["blackbox/queries_median"] == float(np.median(q))
    assert rep["blackbox/stopped_early"] == float((q < 10).mean())
    assert 0.0 <= rep["adv_eval/accuracy"] <= 100.0
