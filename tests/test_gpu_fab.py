"""`-m gpu`: the FAB kernels (include/advstep_fab.h) through the C ABI against the float64 oracle (oracle/fab.py, pinned
to the reference in tests/test_oracle_golden.py) and against the reference's own outputs (tests/golden/fab_*.npz).

Floating-point parity; every tolerance is stated where it is used.  The kernels solve each row's projection without
sorting (fixed-point iteration / bit-wise key bisection), the oracle from sorted breakpoints in float64, the reference
with float32 sort + cumsum + bisection: three summation orders of the same piecewise-linear equation."""
import numpy as np
import pytest
import torch

from oracle import fab as OF
from oracle import torch_ops as O
from oracle.checked_ops import CheckedOps
from tests.helpers import fab_projection_inputs, surrogate_from

pytestmark = pytest.mark.gpu
NORMS = ("Linf", "L2", "L1")
# max-abs on d (moves are <= 1): Linf / L2 a few float32 ulps of the level.  L1's one partially moved coordinate is
# residual / w_i: the residual is a float32 running sum of magnitude ~2e2 at T = 64 600 (ulp 1.5e-5) divided by
# |w_i| ~ 1e-2, so float32 itself — the reference's float32 `s` included — resolves it to a few 1e-3 only
TOL = {"Linf": 2e-5, "L2": 2e-5, "L1": 8e-3}


@pytest.fixture(scope="module")
def ops(cuda):
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def _norm_of(d, norm):
    return OF.row_norm(torch.from_numpy(np.asarray(d, dtype=np.float64)), norm).numpy()


@pytest.mark.parametrize("T", [257, 4099, 64600])
def test_projection_matches_oracle_and_reference(cuda, ops, golden, T):
    g = golden("fab_projection")
    t, w, b = fab_projection_inputs(T, int(g[f"T{T}_seed"]))
    for norm in NORMS:
        d, dn = ops.fab_projection(t.to(cuda), w.to(cuda), b.to(cuda), norm)
        d, dn = d.cpu().numpy(), dn.cpu().numpy()
        want = OF.PROJECTIONS[norm](t.numpy(), w.numpy(), b.numpy())
        ref = g[f"T{T}_{norm.lower()}"]
        # fixed-order reductions, no atomics: a second launch reproduces the first bit for bit
        assert np.array_equal(d, ops.fab_projection(t.to(cuda), w.to(cuda), b.to(cuda), norm)[0].cpu().numpy())
        assert np.abs(d - want).max() <= TOL[norm], (norm, np.abs(d - want).max())
        assert np.abs(d - ref).max() <= TOL[norm], (norm, np.abs(d - ref).max())
        assert np.allclose(dn, _norm_of(want, norm), rtol=1e-4, atol=TOL[norm])
        # structure: coordinates with a zero normal never move; points stay inside the box
        assert (d[:, ::13] == 0).all()
        assert ((t.numpy() + d) >= -1e-6).all() and ((t.numpy() + d) <= 1 + 1e-6).all()
        # the moved point lies on the hyperplane whenever the box lets it (rows 0-4; row 5 is out of reach)
        resid = ((w.double() * (t.double() + torch.from_numpy(d).double())).sum(1) - b.double()).abs().numpy()
        scale = w.abs().sum(1).numpy()
        assert (resid[:5] <= 2e-5 * scale[:5] + TOL[norm] * np.abs(w.numpy()).max()).all(), (norm, resid, scale)


@pytest.mark.parametrize("norm", NORMS)
def test_projection_shared_normals_and_scale(cuda, ops, norm):
    """cat((w, w), 0) is never built: R = 2 * w_rows rows read w[r % w_rows] * wscale[r % w_rows]."""
    gen = torch.Generator().manual_seed(3)
    bs, T = 5, 2048
    pts = torch.rand(2 * bs, T, generator=gen)
    gz = torch.randn(bs, T, generator=gen) * 0.02
    wscale = torch.tensor([2.0, -2.0, 2.0, 0.0, -2.0])
    b = torch.randn(2 * bs, generator=gen) * 0.5
    d, dn = ops.fab_projection(pts.to(cuda), gz.to(cuda), b.to(cuda), norm, wscale.to(cuda))
    w_full = (gz * wscale[:, None]).repeat(2, 1)
    want = OF.PROJECTIONS[norm](pts.numpy(), w_full.numpy(), b.numpy())
    assert np.abs(d.cpu().numpy() - want).max() <= TOL[norm]
    assert (d.cpu().numpy()[[3, 8]] == 0).all() and (dn.cpu().numpy()[[3, 8]] == 0).all()   # zero normal: no move


@pytest.mark.parametrize("norm", NORMS)
def test_projection_edge_rows(cuda, ops, norm):
    """Already on the hyperplane, saturated points (exact 0 / 1), ties in |w|, a single coordinate, empty batch."""
    T = 515   # odd length: scalar path
    gen = torch.Generator().manual_seed(9)
    t = torch.rand(4, T, generator=gen)
    t[1] = (t[1] > 0.5).float()                       # every coordinate sits on a box face
    w = torch.randn(4, T, generator=gen) * 0.05
    w[2] = w[2].sign() * 0.03                          # all |w| equal: L1's tie group is the whole row
    b = (w * t).sum(1)
    b[1] += 0.2
    b[2] -= 0.4
    b[3] += 1e-7
    d, dn = ops.fab_projection(t.to(cuda), w.to(cuda), b.to(cuda), norm)
    want = OF.PROJECTIONS[norm](t.numpy(), w.numpy(), b.numpy())
    got = d.cpu().numpy()
    if norm == "L1":
        # with equal |w| the L1 optimum is not unique coordinate-wise (any order of the tie group is optimal); the kernel
        # and the oracle both take index order, compare the size of the move and the hyperplane residual
        assert np.allclose(np.abs(got).sum(1), np.abs(want).sum(1), rtol=1e-4, atol=1e-4)
    else:
        assert np.abs(got - want).max() <= TOL[norm]
    assert np.abs(got[0]).max() <= 1e-5                # row 0 is on the hyperplane already
    one = ops.fab_projection(torch.tensor([[0.25]], device=cuda), torch.tensor([[2.0]], device=cuda),
                             torch.tensor([1.0], device=cuda), norm)[0]
    assert abs(one.item() - 0.25) <= 1e-6              # 2 * (0.25 + d) = 1
    e, en = ops.fab_projection(torch.empty(0, 8, device=cuda), torch.empty(1, 8, device=cuda), torch.empty(0, device=cuda), norm)
    assert e.shape == (0, 8) and en.shape == (0,)


@pytest.mark.parametrize("norm", NORMS)
def test_hyperplane_matches_oracle(cuda, ops, norm):
    gen = torch.Generator().manual_seed(4)
    B, T = 7, 64600
    gz = torch.randn(B, T, generator=gen) * 1e-3
    x = torch.rand(B, T, generator=gen)
    z = torch.tensor([2.5, -1.0, 0.0, 1e-3, -30.0, 4.0, float("inf")])
    la = torch.tensor([1, 0, 1, 0, 0, 0, 1])
    got = ops.fab_hyperplane(gz.to(cuda), x.to(cuda), z.to(cuda), la.to(cuda), norm)
    want = O.fab_hyperplane(gz, x, z, la, norm)
    for name, a, c in zip(("wscale", "b", "gnorm", "gdot"), got, want):
        a, c = a.cpu().numpy(), c.numpy()
        if name in ("wscale",):
            assert np.array_equal(a, c), name
        else:
            fin = np.isfinite(c)
            assert np.allclose(a[fin], c[fin], rtol=2e-5, atol=2e-5), (name, a, c)
            assert np.array_equal(np.isfinite(a), fin)
    # the selected column is always the OTHER class: wscale = +2 for label 0, -2 for label 1 (fab.py:108-110,225)
    assert got[0].cpu().tolist()[:6] == [-2.0, 2.0, -2.0, 2.0, 2.0, 2.0]
    # statistics only
    _, _, gn, gd = ops.fab_hyperplane(gz.to(cuda), x.to(cuda), None, None, norm)
    assert torch.equal(gn, got[2]) and torch.equal(gd, got[3])


def test_combine_is_bit_exact(cuda, ops):
    gen = torch.Generator().manual_seed(6)
    B, T = 5, 4099
    x1, x0 = torch.rand(B, T, generator=gen), torch.rand(B, T, generator=gen)
    d1, d2 = torch.randn(B, T, generator=gen) * 0.1, torch.randn(B, T, generator=gen) * 0.1
    n1 = torch.tensor([0.3, 0.0, 1e-9, 5.0, 0.2])
    n2 = torch.tensor([0.1, 0.0, 2.0, 1e-3, 0.2])
    for eta, amax in ((1.05, 0.1), (10.0, 0.1), (20.0, 0.5)):
        want = O.fab_combine(x1, x0, d1, d2, n1, n2, eta, amax)
        got = ops.fab_combine(*(v.to(cuda) for v in (x1, x0, d1, d2, n1, n2)), eta, amax)
        assert torch.equal(got.cpu(), want)
    buf = x1.to(cuda)
    assert ops.fab_combine(buf, x0.to(cuda), d1.to(cuda), d2.to(cuda), n1.to(cuda), n2.to(cuda), 1.05, 0.1, out=buf) is buf
    assert torch.equal(buf.cpu(), O.fab_combine(x1, x0, d1, d2, n1, n2, 1.05, 0.1))


@pytest.mark.parametrize("norm", NORMS)
def test_backward_step_matches_oracle(cuda, ops, norm):
    gen = torch.Generator().manual_seed(8)
    B, T = 6, 64600
    x0 = torch.rand(B, T, generator=gen)
    x1 = (x0 + torch.randn(B, T, generator=gen) * 0.01).clamp(0, 1)
    adv = torch.rand(B, T, generator=gen)
    big = float(OF.row_norm(x1 - x0, norm).max()) * 2
    res2 = torch.tensor([1e10, 1e-6, big, 1e10, 1e-6, big])
    flags = torch.tensor([1, 1, 1, 0, 0, 1], dtype=torch.uint8)
    c1, ca, cr = x1.clone(), adv.clone(), res2.clone()
    O.fab_backward_step(c1, x0, ca, cr, flags, 0.9, norm)
    g1, ga, gr = x1.to(cuda), adv.to(cuda), res2.to(cuda)
    ops.fab_backward_step(g1, x0.to(cuda), ga, gr, flags.to(cuda).bool(), 0.9, norm)
    assert torch.equal(g1.cpu(), c1) and torch.equal(ga.cpu(), ca)
    assert torch.allclose(gr.cpu(), cr, rtol=1e-5)
    # rows 3, 4 were not adversarial: untouched; row 1 was adversarial but farther than its best: only steps back
    assert torch.equal(g1.cpu()[3:5], x1[3:5]) and torch.equal(ga.cpu()[[1, 3, 4]], adv[[1, 3, 4]])
    assert torch.equal(ga.cpu()[[0, 2, 5]], x1[[0, 2, 5]])


def test_fab_matches_reference_runs(cuda, golden):
    """Whole FAB runs on the GPU, every kernel launch checked against the oracle in situ, against the reference's own
    adversarial waveforms (eta = 1.05: 2e-5 max-abs after 8-12 iterations through GPU conv arithmetic)."""
    from audio_deepfake_adversarial_attacks_amd import hip_ops, torchattacks
    g = golden("fab_attack")
    model = surrogate_from(g).to(cuda)
    x01, y = torch.from_numpy(g["x01"]).to(cuda), torch.from_numpy(g["labels"]).to(cuda)
    for name, norm in (("linf", "Linf"), ("linf_tight", "Linf"), ("l2", "L2")):
        eta, steps, eps = g[f"{name}_params"]
        atk = torchattacks.FAB(model, norm=norm, n_classes=2, eta=float(eta), steps=int(steps), eps=float(eps))
        atk.ops = CheckedOps(hip_ops)
        atk.set_training_mode(True, False, False)
        adv = atk(x01, y)
        assert atk.ops.calls["fab_projection"] == int(steps) and atk.ops.calls["fab_backward_step"] == int(steps)
        assert (adv.cpu() - torch.from_numpy(g[f"{name}_adv"])).abs().max() <= 2e-5, name
        assert torch.equal(adv[2], x01[2])
        run = atk.attack_single_run(x01, y)
        assert (run.cpu() - torch.from_numpy(g[f"{name}_single_run"])).abs().max() <= 2e-5, name


def test_fab_iterations_replay_reference_trace(cuda, golden):
    """From the reference's x1 at iteration k, one GPU iteration lands on its x1 at k + 1 (2e-5), including
    AttackEnum.FAB's eta = 10."""
    from audio_deepfake_adversarial_attacks_amd import hip_ops, torchattacks
    g = golden("fab_attack")
    model = surrogate_from(g).to(cuda)
    x01, y = torch.from_numpy(g["x01"]).to(cuda), torch.from_numpy(g["labels"]).to(cuda)
    rows = torch.tensor([0, 1, 3, 4, 5], device=cuda)
    x0, la = x01[rows].contiguous(), y[rows].contiguous()
    for name in ("linf", "linf_eta10"):
        eta = float(g[f"{name}_params"][0])
        atk = torchattacks.FAB(model, n_classes=2, eta=eta)
        trace = torch.from_numpy(g[f"{name}_x1"]).to(cuda)
        adv, res2 = x0.clone(), torch.full((5,), 1e10, device=cuda)
        for k in range(trace.shape[0] - 1):
            x1 = trace[k].clone()
            z, gz = atk._logit_and_gradient(x1)
            wscale, b, _, _ = hip_ops.fab_hyperplane(gz, x1, z, la, "Linf")
            d3, n3 = hip_ops.fab_projection(torch.cat((x1, x0)), gz, b.repeat(2), "Linf", wscale)
            hip_ops.fab_combine(x1, x0, d3[:5], d3[5:], n3[:5], n3[5:], eta, 0.1, out=x1)
            flags = atk._get_predicted_label(x1) != la
            hip_ops.fab_backward_step(x1, x0, adv, res2, flags, 0.9, "Linf")
            assert (x1 - trace[k + 1]).abs().max() <= 2e-5, (name, k, (x1 - trace[k + 1]).abs().max().item())


@pytest.mark.parametrize("norm,eps", [("Linf", 0.05), ("L2", 4.0), ("L1", 400.0)])
def test_fab_on_lcnn_invariants(cuda, norm, eps):
    """FAB on LCNN + LFCC at the repo's T = 64 600 (SURVEY 8-d config shapes): size-independent properties."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.utils import to_minmax
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    from audio_deepfake_adversarial_attacks_amd.models.models import get_model
    torch.manual_seed(0)
    model = get_model("lcnn", {"frontend_algorithm": ["lfcc"], "input_channels": 1}, str(cuda)).to(cuda).eval()
    x, _ = synthetic_waveforms(6, 64600)
    x01, _, _ = to_minmax(x.to(cuda))
    with torch.no_grad():
        pred = (model(x01).reshape(-1) > 0).long()
    y = pred.clone()
    y[4] = 1 - y[4]                                       # one utterance the detector already gets wrong
    atk = torchattacks.FAB(model, norm=norm, n_classes=2, eta=1.05, steps=10, eps=eps)
    atk.set_training_mode(True, False, False)
    adv = atk(x01, y)
    assert adv.shape == x01.shape and adv.min() >= 0 and adv.max() <= 1 and torch.isfinite(adv).all()
    assert torch.equal(adv[4], x01[4])
    with torch.no_grad():
        now = (model(adv).reshape(-1) > 0).long()
    size = OF.row_norm((adv - x01).cpu(), norm)
    for r in range(6):
        if r == 4:
            continue
        moved = bool((adv[r] != x01[r]).any())
        # a row is changed only if the change fools the detector within eps (fab.py:515-526)
        assert (not moved) or (now[r] != y[r] and size[r] <= eps * (1 + 1e-5)), (r, size[r].item())


@pytest.mark.parametrize("T", [4, 5])
def test_rows_beyond_one_grid(cuda, ops, T):
    """65 537 rows: the grid holds 65 535 workgroups, so the last two rows are the second trip of each kernel's
    `row += gridDim.x` loop.  T = 4 is the float4 path, T = 5 the scalar one."""
    R = 65537
    ends = [0, 1, R - 3, R - 2, R - 1]
    gen = torch.Generator().manual_seed(11 + T)
    t = torch.rand(R, T, generator=gen)                 # fab_projection_inputs' rows, one offset per row in turn
    t[:, ::7] = 0.0
    t[:, 3::11] = 1.0
    w = torch.randn(R, T, generator=gen) * 0.01
    w[:, ::13] = 0.0
    b = (w * t).sum(1) + torch.tensor([1e-4, -1e-3, 0.05, -0.2, 0.45, 5.0])[torch.arange(R) % 6] * w.abs().sum(1)
    for norm in NORMS:
        out = torch.full((R, T), float("nan"), device=cuda)
        d, dn = ops.fab_projection(t.to(cuda), w.to(cuda), b.to(cuda), norm, out=out)
        d, dn = d.cpu().numpy(), dn.cpu().numpy()
        assert not np.isnan(d).any(), (norm, np.flatnonzero(np.isnan(d).any(1)))
        want = OF.PROJECTIONS[norm](t[ends].numpy(), w[ends].numpy(), b[ends].numpy())
        assert np.abs(d[ends] - want).max() <= TOL[norm], (norm, np.abs(d[ends] - want).max(1))
        assert np.allclose(dn[ends], _norm_of(want, norm), rtol=1e-4, atol=TOL[norm])
        # every row's norm is that of the row beside it: at most T float32 additions, or an exact maximum
        assert np.allclose(dn, _norm_of(d, norm), rtol=1e-5, atol=0), norm

    x1, x0 = torch.rand(R, T, generator=gen), torch.rand(R, T, generator=gen)
    d1, d2 = torch.randn(R, T, generator=gen) * 0.1, torch.randn(R, T, generator=gen) * 0.1
    n1, n2 = torch.rand(R, generator=gen), torch.rand(R, generator=gen)
    n1[::5] = 0.0
    out = torch.full((R, T), float("nan"), device=cuda)
    got = ops.fab_combine(*(v.to(cuda) for v in (x1, x0, d1, d2, n1, n2)), 1.05, 0.1, out=out).cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got, O.fab_combine(x1, x0, d1, d2, n1, n2, 1.05, 0.1))

    x1 = (x0 + torch.randn(R, T, generator=gen) * 0.01).clamp(0, 1)
    adv = torch.rand(R, T, generator=gen)
    flags = torch.tensor([1, 1, 1, 0, 0, 1], dtype=torch.uint8)[torch.arange(R) % 6]
    flags[R - 2:] = 1                                   # the rows of the second trip do work
    for norm in NORMS:
        big = float(OF.row_norm(x1 - x0, norm).max()) * 2
        res2 = torch.tensor([1e10, 1e-6, big, 1e10, 1e-6, big])[torch.arange(R) % 6]
        c1, ca, cr = x1.clone(), adv.clone(), res2.clone()
        O.fab_backward_step(c1, x0, ca, cr, flags, 0.9, norm)
        g1, ga, gr = x1.to(cuda), adv.to(cuda), res2.to(cuda)
        ops.fab_backward_step(g1, x0.to(cuda), ga, gr, flags.to(cuda).bool(), 0.9, norm)
        assert torch.equal(g1.cpu(), c1) and torch.equal(ga.cpu(), ca), norm
        assert torch.allclose(gr.cpu(), cr, rtol=1e-5), norm
        # row R - 2 (best so far 1e10) is kept as the new best and steps back, row R - 1 (1e-6) only steps back
        assert (g1.cpu()[R - 2:] != x1[R - 2:]).any(1).all() and torch.equal(ga.cpu()[R - 2], x1[R - 2])
