"""GPU: randomized smoothing — smooth_noise against the float64 twin (tests/smooth_cpu_ops.py) within a measured bound and against
itself bit for bit (chunks, routes, streams, the counter's carry), its edges and EINVAL cases through the C ABI; smooth_tally
against the twin exactly; torchattacks.Smoothing on the analytic linear case, exact against a recount of the device's own noisy
copies and sound against the closed-form radii; the `certified/*` figures of the evaluation loop."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy import stats

from tests import smooth_cpu_ops as S
from tests.test_gpu_momentum import padded, untouched
from tests.test_gpu_spsa import bits, on_side_stream

pytestmark = pytest.mark.gpu

SEED = (0x01234567 << 32) | 0x89ABCDEF            # non-zero high words
OFFSET = (5 << 32) | 0x00000100
SIGMA = 0.05
FILL = 3.5
# max |out - twin64| / sigma measured on a (16, 65 536), 8-slot fill (tools/smooth_probe.py --error;
# profiles/smooth_noise_timing.txt): the hardware logarithm, sine and cosine behind Box-Muller.  The bound of a sample is twice
# that, times sigma, plus one float32 ulp of the sample for the final add.  The measurement had to come out at most 1e-5.
MEASURED_OVER_SIGMA = 2.6e-6
assert 0.0 < MEASURED_OVER_SIGMA <= 1e-5


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def raw():
    from audio_deepfake_adversarial_attacks_amd import _lib
    return _lib.load()


def stream(cuda):
    return torch.cuda.current_stream(cuda).cuda_stream


def wave(B, T, seed):
    return torch.rand(B, T, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0


def shifted(t, cuda):
    """`t` on the device from a base one float off a 16-byte boundary: the sample-by-sample route at any T."""
    buf = torch.empty(t.numel() + 1, device=cuda)[1:].view(t.shape)
    assert buf.data_ptr() % 16 == 4
    buf.copy_(t)
    return buf


# ---- the noise against the float64 twin -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,off_by_one", [(3, 4099, False), (2, 4100, False), (1, 1, False), (2, 5, False), (2, 4096, True)],
                         ids=["scalar_tile_edge", "vector_tile_edge", "one_sample", "two_quads", "aligned_size_scalar_route"])
def test_noise_against_the_float64_twin(cuda, B, T, off_by_one):
    ops, ns, s0 = hip(), 3, 2
    x = wave(B, T, 100 + T)
    x_d = shifted(x, cuda) if off_by_one else x.to(cuda)
    buf, out = padded((ns, B, T), FILL, cuda)
    assert ops.smooth_noise(x_d, SIGMA, SEED, OFFSET, s0=s0, ns=ns, out=out) is out
    torch.cuda.synchronize()
    assert untouched(buf, FILL, ns * B * T)                                          # a canary either side of `out`
    got = out.cpu().numpy().astype(np.float64)
    twin = S.smooth_noise_np(x, SIGMA, SEED, OFFSET, s0, ns, dtype=np.float64)
    err = np.abs(got - twin)
    bound = 2.0 * MEASURED_OVER_SIGMA * float(np.float32(SIGMA)) + np.spacing(np.abs(twin).astype(np.float32)).astype(np.float64)
    print(f"({B}, {T}): max |out - twin64| / sigma = {err.max() / SIGMA:.3e}, largest share of the bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert np.abs(got - x.numpy()[None]).max() > SIGMA                                # it IS noise: some sample moved by more than sigma
    assert torch.equal(bits(x_d), bits(x))                                            # the input is read only


# ---- bit-identity -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [4100, 4099])
def test_chunks_routes_and_streams_give_the_same_bits(cuda, T):
    ops, B, ns = hip(), 3, 5
    x = wave(B, T, 7)
    x_d = x.to(cuda)
    whole = ops.smooth_noise(x_d, SIGMA, SEED, OFFSET, s0=1, ns=ns)
    assert whole.shape == (ns, B, T)
    parts = torch.cat([ops.smooth_noise(x_d, SIGMA, SEED, OFFSET, s0=1, ns=2), ops.smooth_noise(x_d, SIGMA, SEED, OFFSET, s0=3, ns=3)])
    assert torch.equal(bits(parts), bits(whole))                                      # a fill in chunks, 2 + 3
    moved = torch.cat([ops.smooth_noise(x_d, SIGMA, SEED, OFFSET + 1, s0=0, ns=2), ops.smooth_noise(x_d, SIGMA, SEED, OFFSET + 3, s0=0, ns=3)])
    assert torch.equal(bits(moved), bits(whole))                                      # only offset + s enters
    assert torch.equal(bits(ops.smooth_noise(shifted(x, cuda), SIGMA, SEED, OFFSET, s0=1, ns=ns)), bits(whole))   # the scalar route
    other = on_side_stream(cuda, lambda: ops.smooth_noise(x_d, SIGMA, SEED, OFFSET, s0=1, ns=ns))
    assert torch.equal(bits(other), bits(whole))                                      # a rerun, on a second stream
    for seed, offset in ((SEED + 1, OFFSET), (SEED ^ (1 << 50), OFFSET), (SEED, OFFSET ^ (1 << 40))):
        assert not torch.equal(ops.smooth_noise(x_d, SIGMA, seed, offset, s0=1, ns=ns), whole)
    assert not torch.equal(whole[0], whole[1])


def test_the_counter_carries_into_its_high_word(cuda):
    ops = hip()
    x_d = wave(2, 260, 3).to(cuda)
    base = 2 ** 32 - 2
    whole = ops.smooth_noise(x_d, SIGMA, SEED, base, s0=0, ns=4)
    singles = torch.cat([ops.smooth_noise(x_d, SIGMA, SEED, base + i, s0=0, ns=1) for i in range(4)])
    assert torch.equal(bits(whole), bits(singles))
    assert not torch.equal(whole[2], ops.smooth_noise(x_d, SIGMA, SEED, 0, s0=0, ns=1)[0])   # 2^32 is not 0: the high word counts
    twin = S.smooth_noise_np(x_d, SIGMA, SEED, base, 0, 4, dtype=np.float64)
    assert np.abs(whole.cpu().numpy() - twin).max() <= 2.0 * MEASURED_OVER_SIGMA * SIGMA + 2.0 ** -23


def test_sigma_zero_returns_x(cuda):
    ops = hip()
    x = wave(2, 4100, 9)
    x[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    out = ops.smooth_noise(x.to(cuda), 0.0, SEED, OFFSET, ns=2)
    assert bool((out.cpu() == x[None]).all())                                         # == (not bytes: -0 + 0 is +0)


# ---- edges ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [4100, 4099])
def test_nan_stays_and_its_neighbours_are_untouched(cuda, T):
    ops = hip()
    x = wave(2, T, 21)
    clean = ops.smooth_noise(x.to(cuda), SIGMA, SEED, OFFSET, ns=2).cpu()
    holes = [(0, 0), (0, 4097), (1, 1), (1, T - 1)]
    for b, t in holes:
        x[b, t] = float("nan")
    got = ops.smooth_noise(x.to(cuda), SIGMA, SEED, OFFSET, ns=2).cpu()
    mask = torch.zeros(2, T, dtype=torch.bool)
    for b, t in holes:
        mask[b, t] = True
    assert bool(torch.isnan(got[:, mask]).all()) and int(torch.isnan(got).sum()) == 2 * len(holes)
    assert torch.equal(bits(got[:, ~mask]), bits(clean[:, ~mask]))


@pytest.mark.parametrize("B,T,ns", [(0, 8, 2), (3, 0, 2), (3, 8, 0)])
def test_empty_sizes_write_nothing(cuda, B, T, ns):
    lib = raw()
    x = torch.zeros(32, device=cuda)
    canary = torch.full((256,), FILL, device=cuda)
    assert lib.advstep_smooth_noise_f32(x.data_ptr(), canary.data_ptr(), B, T, 0, ns, SIGMA, 1, 0, stream(cuda)) == 0
    assert lib.advstep_smooth_noise_f32(None, None, B, T, 0, ns, SIGMA, 1, 0, stream(cuda)) == 0   # null pointers are fine then
    torch.cuda.synchronize()
    assert bool((canary == FILL).all())
    if B and ns:                                                                      # the wrapper: an empty result, nothing launched
        assert hip().smooth_noise(torch.zeros(B, T, device=cuda), SIGMA, 1, ns=ns).shape == (ns, B, T)


def test_every_einval_case_of_the_header(cuda):
    lib, EINVAL = raw(), 1
    x = torch.zeros(2, 8, device=cuda)
    out = torch.full((3, 2, 8), FILL, device=cuda)
    st = stream(cuda)

    def noise(xp=x.data_ptr(), op=out.data_ptr(), B=2, T=8, s0=0, ns=3, sigma=SIGMA):
        return lib.advstep_smooth_noise_f32(xp, op, B, T, s0, ns, sigma, 1, 0, st)

    assert noise(B=-1) == EINVAL and noise(T=-1) == EINVAL and noise(ns=-1) == EINVAL and noise(s0=-1) == EINVAL
    assert noise(B=65_536) == EINVAL
    assert noise(xp=None) == EINVAL and noise(op=None) == EINVAL
    assert noise(op=x.data_ptr()) == EINVAL and noise(xp=out.data_ptr() + 4 * 40) == EINVAL   # out overlaps x
    for sigma in (-0.01, float("nan"), float("inf"), -float("inf")):
        assert noise(sigma=sigma) == EINVAL
    z = torch.zeros(3, 2, device=cuda)
    counts = torch.full((2,), 7, dtype=torch.int32, device=cuda)

    def tally(zp=z.data_ptr(), cp=counts.data_ptr(), B=2, ns=3):
        return lib.advstep_smooth_tally_i32(zp, cp, B, ns, st)

    assert tally(B=-1) == EINVAL and tally(ns=-1) == EINVAL and tally(zp=None) == EINVAL and tally(cp=None) == EINVAL
    assert tally(cp=z.data_ptr()) == EINVAL
    assert tally(B=0) == 0 and tally(ns=0) == 0 and tally(zp=None, cp=None, ns=0) == 0
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and counts.tolist() == [7, 7]                    # nothing was launched
    ops = hip()
    with pytest.raises(ValueError, match="sigma"):
        ops.smooth_noise(x, -1.0, 1)
    with pytest.raises(ValueError, match="s0 and ns"):
        ops.smooth_noise(x, 0.1, 1, s0=-1)
    with pytest.raises(ValueError, match="out must hold"):
        ops.smooth_noise(x, 0.1, 1, ns=2, out=torch.zeros(3, 2, 8, device=cuda))
    with pytest.raises(TypeError, match="int32"):
        ops.smooth_tally(z, counts.long())
    with pytest.raises(ValueError, match="one value per row"):
        ops.smooth_tally(z, torch.zeros(3, dtype=torch.int32, device=cuda))


# ---- the tally -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 7, 130])
@pytest.mark.parametrize("ns", [0, 1, 33])
def test_tally_is_the_twins(cuda, B, ns):
    ops = hip()
    g = torch.Generator().manual_seed(B * 100 + ns)
    special = torch.tensor([float("nan"), 0.0, -0.0, float("inf"), -float("inf"), 1e-45, -1e-45, 1e-38, -1e-38, 1.0, -1.0])
    z = special[torch.randint(0, special.numel(), (ns, B), generator=g)]
    z2 = torch.randn(ns, B, generator=g)
    start = torch.randint(0, 1000, (B,), generator=g).to(torch.int32)
    buf = torch.full((B + 64,), 77, dtype=torch.int32, device=cuda)
    counts = buf[32:32 + B]
    counts.copy_(start)
    assert ops.smooth_tally(z.to(cuda), counts) is counts
    want = S.smooth_tally_np(z, start)
    assert np.array_equal(counts.cpu().numpy(), want)
    ops.smooth_tally(z2.to(cuda), counts)                                             # it accumulates over two calls
    assert np.array_equal(counts.cpu().numpy(), S.smooth_tally_np(z2, want))
    assert bool((buf[:32] == 77).all() and (buf[32 + B:] == 77).all())
    if ns == 33:
        assert want.max() > start.numpy().min() and (S.smooth_tally_np(z, np.zeros(B, np.int32)) < ns).all()   # NaN, zeros and negatives did not count


# ---- the procedure on the analytic case ---------------------------------------------------------------------------------------------------

N, N0, ALPHA, PSEED, POFFSET, MAX_ROWS = 1024, 64, 0.001, 1234, 5, 200


@pytest.fixture(scope="module", params=[1028, 1030])
def certified(request):
    """Smoothing.certify on linear_case(T), run once per T: max_rows = 200 at B = 8 gives fills of 25 slots, so the 64
    selection slots go as 25 + 25 + 14 and the 1024 estimation slots as 40 x 25 + 24."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    cuda = torch.device("cuda:0")
    model, x, y, k, sigma = S.linear_case(request.param)
    sm = torchattacks.Smoothing(sigma, n=N, n0=N0, alpha=ALPHA, max_rows=MAX_ROWS, seed=PSEED)
    assert MAX_ROWS // 8 == 25 and N0 % 25 and N % 25
    rows = sm.certify(model.to(cuda), x.to(cuda), POFFSET)
    torch.cuda.synchronize()
    return SimpleNamespace(T=request.param, model=model.cpu(), x=x, y=y, k=k, sigma=sigma, sm=sm, rows=rows.cpu().numpy())


def test_certify_equals_a_recount_of_the_devices_own_copies(cuda, certified):
    """The device's noisy copies at the documented offsets (selection: POFFSET .. + n0 - 1, estimation: the n after them), copied
    to the CPU and scored there by the float64 model: class and kA are exactly the recount's.  The float32 transcendentals are on
    both sides of the comparison; what it pins is chunking, offsets, selection, ties and the tally."""
    c, ops = certified, hip()
    assert c.rows.shape == (8, 2) and c.rows.dtype == np.int32
    x_d = c.x.to(cuda)

    def recount(offset, m):
        copies = ops.smooth_noise(x_d, c.sigma, PSEED, offset, s0=0, ns=m).cpu()
        z64 = copies.double() @ c.model.w.detach() + c.model.bias                     # (m, 8)
        assert float(z64.abs().min()) > 1e-9                                          # precondition: no logit at the boundary
        return (z64.float() > 0).sum(dim=0).numpy()

    c0, c1 = recount(POFFSET, N0), recount(POFFSET + N0, N)
    cls = (2 * c0 > N0).astype(np.int32)
    assert np.array_equal(c.rows[:, 0], cls)
    assert np.array_equal(c.rows[:, 1], np.where(cls == 1, c1, N - c1))
    pred = c.sm.predict(c.model.to(cuda), x_d, POFFSET).cpu().numpy()                # PREDICT: the same selection votes
    c.model.cpu()
    assert np.array_equal(pred[:, 0], c0) and (pred[:, 1] == N0).all()


def test_certificates_are_sound_on_the_linear_detector(certified):
    """Row b's true L2 radius is |k_b| sigma.  Every certified radius is at most that; the k = 0 row abstains; rows with
    |k| >= 0.5 are certified for the right class with at least 0.6 |k| sigma."""
    from audio_deepfake_adversarial_attacks_amd import metrics
    c = certified
    radius = np.asarray(metrics.certified_radius(c.rows[:, 1], N, ALPHA, c.sigma))
    k = c.k.numpy()
    print(f"T = {c.T}: radius / sigma = {np.round(radius / c.sigma, 3).tolist()} for k = {k.tolist()}")
    assert (radius <= np.abs(k) * c.sigma).all()
    assert radius[k == 0.0] == -1.0
    strong = np.abs(k) >= 0.5
    assert (c.rows[strong, 0] == c.y.numpy()[strong]).all()
    assert (radius[strong] >= 0.6 * np.abs(k[strong]) * c.sigma).all()


def test_scorer_counts_no_violation_inside_the_certified_radius(cuda, certified):
    """Through evaluation._CertifyScorer: each certified row is pushed straight at the boundary by HALF its certified radius (a
    hand-made waveform perturbation of that L2); the smoothed detector's PREDICT must not flip: violations == 0."""
    from audio_deepfake_adversarial_attacks_amd import evaluation, metrics
    c = certified
    radius = np.asarray(metrics.certified_radius(c.rows[:, 1], N, ALPHA, c.sigma))
    w = c.model.w.detach()
    toward = torch.where(torch.from_numpy(c.rows[:, 0]) == 1, -1.0, 1.0).double()     # class 1 moves against w
    step = torch.from_numpy(np.where(radius > 0, 0.5 * radius, 0.0)).double()
    attacked = (c.x.double() + (toward * step)[:, None] * (w / w.norm())[None]).float()
    scorer = evaluation._CertifyScorer(c.sigma, N, N0, ALPHA, cuda, seed=PSEED, attacked=True)
    scorer.smooth.max_rows = MAX_ROWS
    scorer.offset = POFFSET                                                           # the fixture's certificate again
    model = c.model.to(cuda)
    kept = scorer.scored(0, model, c.x.to(cuda), attacked.to(cuda), c.y.to(cuda), None, None)
    c.model.cpu()
    assert len(kept) == 2 and scorer.offset == POFFSET + N0 + N + N0
    out = scorer.finish(SimpleNamespace(all_y=c.y.numpy(), world=1, rank=0, device=cuda))
    rows = scorer.scores()["certified"]
    assert np.array_equal(rows["class"], c.rows[:, 0]) and np.array_equal(rows["kA"], c.rows[:, 1])
    np.testing.assert_allclose(rows["l2"], step.numpy(), rtol=1e-3, atol=1e-7)        # perturbation_stats' L2 of the hand-made move
    assert out["certified/violations"] == 0 and isinstance(out["certified/violations"], int)
    assert 0.0 <= out["certified/attacked_accuracy"] <= 100.0 and 0.0 <= out["certified/attacked_abstained"] <= 100.0
    spans = (c.x.amax(dim=1) - c.x.amin(dim=1)).numpy()
    np.testing.assert_array_equal(rows["span"], spans)


# ---- through the loop -----------------------------------------------------------------------------------------------------------------------

CFG = {"data": {"seed": 42}, "checkpoint": {"path": ""},
       "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}
CERT_KEYS = ["certified/accuracy", "certified/abstained", "certified/radius_median", "certified/radius_norm_median",
             "certified/accuracy_at_0.1", "certified/accuracy_at_0.15", "certified/accuracy_at_0.2", "certified/radius_max",
             "certified/sigma", "certified/n", "certified/alpha"]
ATTACKED_KEYS = ["certified/attacked_accuracy", "certified/attacked_abstained", "certified/violations"]
CERTIFY = {"certify": 0.05, "certify_samples": 32, "certify_select": 8}


def loop(method, params, **kw):
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks
    torch.manual_seed(5)
    rep = generate_attacks([None, None, None], CFG, "cuda:0", attack_model_config=CFG if method else None, attack_method=method,
                           attack_params=params, batch_size=4, dataset=SyntheticDetectionDataset(8), share_weights=True,
                           shuffle=False, num_workers=0, return_scores=True, **kw)
    torch.cuda.synchronize()
    return rep


def certified_part(rep):
    return {k: v for k, v in rep.items() if k.startswith("certified/")}, rep["scores"]["certified"]


def same_certificates(a, b):
    (ka, ra), (kb, rb) = certified_part(a), certified_part(b)
    np.testing.assert_equal(ka, kb)                                                   # NaN medians compare equal
    assert list(ra) == list(rb) and all(np.array_equal(ra[k], rb[k], equal_nan=True) for k in ra)


def test_loop_without_an_attack(cuda):
    """8 synthetic utterances, batch 4, LCNN + LFCC at random initialisation, sigma 0.05 with 32 + 8 copies: every certified/*
    key, the same figures and rows with one and two batches in flight and on a rerun, and the adv_eval scores of the run
    without `certify`, bit for bit."""
    plain = loop(None, {})
    assert not [k for k in plain if k.startswith("certified/")] and "certified" not in plain["scores"]
    rep = loop(None, {}, in_flight=1, **CERTIFY)
    assert [k for k in rep if k.startswith("certified/")] == CERT_KEYS and rep["num_total"] == 8
    assert rep["certified/accuracy"] + rep["certified/abstained"] <= 100.0 + 1e-9
    assert (rep["certified/sigma"], rep["certified/n"], rep["certified/alpha"]) == (0.05, 32, 0.001)
    assert rep["certified/radius_max"] == pytest.approx(0.05 * stats.norm.ppf(0.001 ** (1 / 32)), abs=1e-12)   # the ceiling of 32 copies
    rows = rep["scores"]["certified"]
    assert list(rows) == ["class", "kA", "radius", "span"] and all(v.shape == (8,) for v in rows.values())
    assert ((rows["kA"] >= 0) & (rows["kA"] <= 32)).all() and set(rows["class"]) <= {0, 1} and (rows["span"] > 0).all()
    same_certificates(rep, loop(None, {}, in_flight=2, **CERTIFY))
    same_certificates(rep, loop(None, {}, in_flight=1, **CERTIFY))
    assert np.array_equal(rep["scores"]["y_pred"], plain["scores"]["y_pred"])
    assert {k: v for k, v in rep.items() if k.startswith("adv_eval/")} == {k: v for k, v in plain.items() if k.startswith("adv_eval/")}


def test_loop_with_pgdl2(cuda):
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    method, params = AttackEnum["PGDL2"].value
    params = {**params, "steps": 2}
    plain = loop(method, params)
    rep = loop(method, params, **CERTIFY)
    assert [k for k in rep if k.startswith("certified/")] == CERT_KEYS + ATTACKED_KEYS
    assert isinstance(rep["certified/violations"], int) and rep["certified/violations"] >= 0
    assert 0.0 <= rep["certified/attacked_accuracy"] <= 100.0 and 0.0 <= rep["certified/attacked_abstained"] <= 100.0
    assert list(rep["scores"]["certified"]) == ["class", "kA", "radius", "span", "attacked_c1", "attacked_class", "l2"]
    assert (rep["scores"]["certified"]["l2"] > 0).all()
    assert np.array_equal(rep["scores"]["y_pred"], plain["scores"]["y_pred"])
    assert {k: v for k, v in rep.items() if k.startswith("adv_eval/")} == {k: v for k, v in plain.items() if k.startswith("adv_eval/")}
