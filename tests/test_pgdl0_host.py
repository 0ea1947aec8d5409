"""CPU: PGDL0's host logic — the public surface, argument validation through the C ABI, the CPU op table (tests/l0_cpu_ops.py)
against a brute-force float64 restatement of the projection's definition on tiny rows, the loop report's digest, and whole
attacks on a tiny linear (B, T) -> (B, 1) model.

The brute-force rows live on the grid of multiples of 1/16 in [-1, 2]: every d, c, r, d^2, r^2 and score is then exact in
float32 and in float64 alike, so the table's float32 result must reach the float64 optimum exactly, with no tolerance."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import l0_cpu_ops as C


class Linear(torch.nn.Module):
    """(B, T) -> (B, 1): one weight per sample."""

    def __init__(self, T, seed=3):
        super().__init__()
        self.fc = torch.nn.Linear(T, 1)
        with torch.no_grad():
            self.fc.weight.copy_(torch.randn(1, T, generator=torch.Generator().manual_seed(seed)) * 0.2)
            self.fc.bias.zero_()

    def forward(self, x):
        return self.fc(x - 0.5)


def test_public_surface_and_enum_members():
    from audio_deepfake_adversarial_attacks_amd import hip_ops, torchattacks
    from audio_deepfake_adversarial_attacks_amd.aa.aa_types import AttackEnum
    assert "PGDL0" in torchattacks.__all__ and torchattacks.PGDL0.__module__.endswith("attacks.pgdl0")
    assert len(set(torchattacks.__all__)) == len(torchattacks.__all__)
    assert callable(hip_ops.l0_box_project) and callable(hip_ops.pgdl0_step)
    names = [m.name for m in AttackEnum]
    assert len(set(names)) == len(names) and len(AttackEnum.__members__) == len(names)      # no member aliases another
    m = Linear(32)
    want = {"PGDL0": {"k": 64, "alpha": 0.15, "steps": 20}, "PGDL0_k256": {"k": 256, "alpha": 0.15, "steps": 20},
            "PGDL0_k1024": {"k": 1024, "alpha": 0.15, "steps": 20},
            "PGDL0_k1024_cap005": {"k": 1024, "alpha": 0.15, "steps": 20, "eps_inf": 0.05}}
    for name, kw in want.items():
        cls, got = AttackEnum[name].value
        assert cls is torchattacks.PGDL0 and got == kw
        atk = cls(m, **got)
        assert (atk.k, atk.alpha, atk.steps, atk.eps_inf, atk.random_start) == (kw["k"], 0.15, 20, kw.get("eps_inf"), True)
        assert atk._supported_mode == ["default", "targeted"] and atk.replays_from_graph and atk.last_changed is None
    assert AttackEnum["PGD"].value[0] is torchattacks.PGD and AttackEnum["NO_ATTACK"].value == (None, {})
    assert str(torchattacks.PGDL0(m, k=3, steps=7)) == (
        "PGDL0(model_name=Linear, device=cpu, k=3, alpha=0.15, steps=7, eps_inf=None, random_start=True, "
        "attack_mode=default, return_type=float)")
    import evaluate_models_on_adversarial_attacks as cli
    for name in want:
        assert cli.parse_arguments(["--attack", name]).attack == name


def test_value_errors():
    from audio_deepfake_adversarial_attacks_amd import hip_ops, torchattacks
    m = Linear(8)
    for kw in ({"k": 0}, {"k": -3}, {"k": 2.5}, {"steps": 0}, {"alpha": 0.0}, {"alpha": -1.0}, {"alpha": float("nan")},
               {"eps_inf": 0.0}, {"eps_inf": -0.1}, {"eps_inf": float("nan")}):
        with pytest.raises(ValueError):
            torchattacks.PGDL0(m, **kw)
    torchattacks.PGDL0(m, k=1, steps=1, alpha=1e-3, eps_inf=math.inf)
    with pytest.raises(ValueError, match="k must"):
        hip_ops._l0_budget(0, math.inf)
    with pytest.raises(ValueError, match="eps_inf"):
        hip_ops._l0_budget(4, 0.0)
    assert hip_ops._l0_budget(4, 0.05) == (4, 0.05)
    x = torch.zeros(2, 8)
    with pytest.raises(Exception, match="HIP device|cpu"):                   # no CPU path in the package
        hip_ops.l0_box_project(x, x, 2)


def test_argument_validation_needs_no_device():
    """Invalid arguments are rejected before any launch, and B = 0 launches nothing (safe without a GPU)."""
    import ctypes

    from audio_deepfake_adversarial_attacks_amd import _lib, build
    build.build()
    lib = _lib.load()
    OK, EINVAL = 0, 1
    inf = math.inf
    p, q, r, s = (ctypes.c_void_p(a) for a in (0x1000, 0x100000, 0x200000, 0x300000))       # never dereferenced
    proj, step = lib.advstep_l0_box_project_f32, lib.advstep_pgdl0_step_f32
    assert proj(p, q, r, 4, inf, 0, 64_600, None) == OK
    assert proj(None, None, None, 4, inf, 0, 0, None) == OK
    assert proj(None, q, r, 4, inf, 2, 8, None) == EINVAL
    assert proj(p, None, r, 4, inf, 2, 8, None) == EINVAL
    assert proj(p, q, None, 4, inf, 2, 8, None) == EINVAL
    assert proj(p, q, p, 4, inf, 2, 8, None) == EINVAL                       # out aliases x
    assert proj(p, q, r, 0, inf, 2, 8, None) == EINVAL                       # k >= 1
    assert proj(p, q, r, -1, inf, 0, 8, None) == EINVAL                      # ... even for an empty batch
    assert proj(p, q, r, 4, 0.0, 2, 8, None) == EINVAL                       # eps_inf > 0
    assert proj(p, q, r, 4, float("nan"), 2, 8, None) == EINVAL
    assert proj(p, q, r, 4, inf, 2, 1 << 24, None) == EINVAL                 # counts are exact floats below 2^24
    assert proj(p, q, r, 4, inf, 2, 0, None) == EINVAL
    assert proj(p, q, r, 4, inf, -1, 8, None) == EINVAL
    assert step(None, None, None, None, None, 1.0, 4, inf, 0, 8, None) == OK
    assert step(None, q, r, s, None, 1.0, 4, inf, 2, 8, None) == EINVAL
    assert step(p, None, r, s, None, 1.0, 4, inf, 2, 8, None) == EINVAL
    assert step(p, q, None, s, None, 1.0, 4, inf, 2, 8, None) == EINVAL
    assert step(p, q, r, None, None, 1.0, 4, inf, 2, 8, None) == EINVAL
    assert step(p, q, r, q, None, 1.0, 4, inf, 2, 8, None) == EINVAL         # out aliases grad
    assert step(p, q, r, r, None, 1.0, 4, inf, 2, 8, None) == EINVAL         # out aliases x
    assert step(p, q, r, s, s, 1.0, 4, inf, 2, 8, None) == EINVAL            # stats inside out
    assert step(p, q, r, s, None, -1.0, 4, inf, 2, 8, None) == EINVAL        # step >= 0
    assert step(p, q, r, s, None, float("nan"), 4, inf, 2, 8, None) == EINVAL
    assert step(p, q, r, s, None, 1.0, 0, inf, 2, 8, None) == EINVAL
    assert step(p, q, r, s, None, 1.0, 4, -0.05, 2, 8, None) == EINVAL
    assert step(p, q, r, s, None, 1.0, 4, inf, 2, 1 << 24, None) == EINVAL
    assert lib.advstep_abi_version() == 3


# ---- the projection against brute force ----------------------------------------------------------------------------------------

def grid_rows(B, T, seed):
    """x in [0, 1] and u in [-1, 2] on multiples of 1/16, with exact 0s and 1s in x and samples where u == x."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 17, (B, T), generator=g).float() / 16.0
    u = torch.randint(-16, 33, (B, T), generator=g).float() / 16.0
    u = torch.where(torch.rand(B, T, generator=g) < 0.2, x, u)
    x[0] = 0.5                                                              # row 0: every score equal, the index rule decides
    u[0] = 0.5 + 0.25 * torch.sign(torch.randn(T, generator=g))
    return x, u


_MASKS = {}


def brute_force(x, u, k, eps_inf):
    """The definition in float64 over every subset of min(k, T) kept coordinates of one row: (least squared distance, the
    minimiser when it is unique else None)."""
    x, u = x.double().numpy(), u.double().numpy()
    T, kk = x.size, min(k, x.size)
    if (T, kk) not in _MASKS:
        masks = np.zeros((math.comb(T, kk), T), dtype=bool)
        for n, keep in enumerate(itertools.combinations(range(T), kk)):
            masks[n, list(keep)] = True
        _MASKS[T, kk] = masks
    z_keep = np.minimum(np.maximum(u, np.maximum(x - eps_inf, 0.0)), np.minimum(x + eps_inf, 1.0))   # a kept coordinate's box projection
    z = np.where(_MASKS[T, kk], z_keep, x)
    dist = ((z - u) ** 2).sum(axis=1)
    best = dist.min()
    args = np.unique(z[dist == best], axis=0)
    return float(best), (torch.from_numpy(args[0]) if len(args) == 1 else None)


@pytest.mark.parametrize("T", [1, 5, 12])
def test_table_projection_is_the_brute_force_optimum(T):
    B = 6
    seen_unique = seen_tied = 0
    for eps_inf in (math.inf, 0.25):
        x, u = grid_rows(B, T, 100 + T)
        for k in range(1, T + 2):
            out = C.l0_box_project(x, u, k, eps_inf)
            assert ((out != x).sum(dim=1) <= k).all()
            assert (out >= torch.clamp(x - eps_inf, min=0.0)).all() and (out <= torch.clamp(x + eps_inf, max=1.0)).all()
            for b in range(B):
                best, arg = brute_force(x[b], u[b], k, eps_inf)
                assert ((out[b].double() - u[b].double()) ** 2).sum().item() == best     # exact on the grid: optimal, ties included
                if arg is not None:
                    assert torch.equal(out[b].double(), arg)
                    seen_unique += 1
                else:
                    seen_tied += 1
    assert seen_unique > 0 and (T == 1 or seen_tied > 0)                     # both kinds of row were met


def test_table_tie_rule_and_stats():
    """Equal scores: the lower index wins, the stats name the threshold, the count above it and the last kept tie."""
    x = torch.full((1, 8), 0.5)
    u = x + torch.tensor([[0.25, -0.25, 0.0, 0.25, 0.375, -0.25, 0.25, 0.0]])
    for k, kept, gt, cut in ((1, [4], 0, 4), (2, [0, 4], 1, 0), (3, [0, 1, 4], 1, 1), (6, [0, 1, 3, 4, 5, 6], 1, 6),
                             (7, [0, 1, 2, 3, 4, 5, 6], 6, 2), (8, list(range(8)), 6, 7), (13, list(range(8)), 6, 7)):
        out, thr, g, c = C.project(x, u, k, return_stats=True)
        want = x.clone()
        want[0, kept] = u[0, kept]
        assert torch.equal(out, want), k
        assert (g.item(), c.item()) == (gt, cut), k
        assert thr.item() == (0.0 if k >= 7 else 0.0625 if k >= 2 else 0.140625)
    # the cap: scores count what keeping saves, d^2 - r^2, not how far u is
    out = C.l0_box_project(x, x + torch.tensor([[1.0, 0.1, 0, 0, 0, 0, 0, -0.2]]), 1, 0.05)
    assert torch.equal(out, x + torch.tensor([[0.05, 0, 0, 0, 0, 0, 0, 0]]))
    # the step with a zero gradient returns a feasible cur; gnorm= replaces the table's own sum
    cur = x.clone()
    cur[0, 3] = 0.75
    got, stats = C.pgdl0_step(cur, torch.zeros(1, 8), x, 1.0, 2, return_stats=True)
    assert torch.equal(got, cur) and stats.tolist() == [[0.0, 0.0, 1.0, 0.0]]
    g = torch.tensor([[1.0, -2.0, 0, 0, 0, 0, 0, 1.0]])
    a = C.pgdl0_step(x, g, x, 0.5, 8)
    b = C.pgdl0_step(x, g, x, 0.5, 8, gnorm=torch.tensor([8.0]))
    assert torch.equal(a, x + 0.5 * g / 4.0) and torch.equal(b, x + 0.5 * g / 8.0)


def test_sparsity_summary():
    from audio_deepfake_adversarial_attacks_amd import evaluation, metrics
    rep = metrics.sparsity_summary([3, 64, 0, 10], 64)
    assert rep == {"sparse/changed_mean": 19.25, "sparse/changed_median": 6.5, "sparse/changed_max": 64, "sparse/k": 64}
    assert isinstance(rep["sparse/changed_max"], int) and isinstance(rep["sparse/k"], int)
    assert metrics.sparsity_summary(np.array([[5], [7]], dtype=np.int64), 8)["sparse/changed_mean"] == 6.0
    empty = metrics.sparsity_summary([], 16)
    assert math.isnan(empty["sparse/changed_mean"]) and math.isnan(empty["sparse/changed_median"])
    assert empty["sparse/changed_max"] == 0 and empty["sparse/k"] == 16
    rep["adv_eval/eer"] = 0.5
    assert evaluation.format_sparse(rep) == ("sparse/changed_mean: 19.25, sparse/changed_median: 6.5, sparse/changed_max: 64, "
                                             "sparse/k: 64")


# ---- whole attacks on the table ----------------------------------------------------------------------------------------------

def _run(k, steps=6, eps_inf=None, random_start=True, noise=None, targeted=False, T=200):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    torch.manual_seed(5)
    m = Linear(T).eval()
    x = torch.rand(6, T, generator=torch.Generator().manual_seed(9)) * 0.5 + 0.25
    x[:, ::11] = 0.0
    x[:, 3::13] = 1.0
    with torch.no_grad():
        y = (m(x).reshape(-1) > 0).to(torch.int64)
    atk = torchattacks.PGDL0(m, k=k, steps=steps, eps_inf=eps_inf, random_start=random_start)
    atk.ops = C
    if noise is not None:
        atk.set_init_noise(noise)
    if targeted:
        atk.set_mode_targeted_by_function(lambda images, labels: 1 - labels)
    return atk, x, y, atk(x, y)


@pytest.mark.parametrize("k,eps_inf", [(1, None), (7, None), (7, 0.05), (200, None), (500, 0.3)])
def test_whole_attack_invariants_on_cpu_table(k, eps_inf):
    atk, x, y, adv = _run(k, eps_inf=eps_inf)
    assert adv.dtype == torch.float32 and adv.shape == x.shape and adv.data_ptr() != x.data_ptr()
    changed = (adv != x).sum(dim=1)
    assert (changed <= k).all() and changed.max() > 0
    assert atk.last_changed.dtype == torch.int64 and torch.equal(atk.last_changed, changed)
    assert adv.min() >= 0 and adv.max() <= 1
    if eps_inf is not None:
        e = torch.tensor(eps_inf, dtype=torch.float32)                      # the cap's bounds as float32 forms them: x -+ eps_inf
        assert (adv <= x + e).all() and (adv >= x - e).all()
    assert torch.equal(adv, _run(k, eps_inf=eps_inf)[3])                     # same seed, same bytes
    # from x itself every kept move follows the (constant) gradient of a linear model: every logit goes the attack's way
    atk, x, y, adv = _run(k, eps_inf=eps_inf, random_start=False)
    assert ((adv != x).sum(dim=1) <= k).all() and adv.min() >= 0 and adv.max() <= 1
    with torch.no_grad():
        z0, z1 = atk.model(x).reshape(-1), atk.model(adv).reshape(-1)
    assert (torch.where(y == 1, z1 < z0, z1 > z0)).all()


def test_starts_modes_and_explicit_draw():
    draw = torch.rand(6, 200, generator=torch.Generator().manual_seed(1)) * 2 - 1
    _, x, y, a1 = _run(5, noise=draw)
    _, _, _, a2 = _run(5, noise=draw)
    assert torch.equal(a1, a2) and ((a1 != x).sum(dim=1) <= 5).all()
    _, _, _, a3 = _run(5, steps=1, random_start=False)
    assert ((a3 != x).sum(dim=1) <= 5).all() and not torch.equal(a3, x)
    atk, _, _, a4 = _run(5, targeted=True, random_start=False)
    with torch.no_grad():                                                   # towards the target 1 - y: away from y all the same
        z0, z1 = atk.model(x).reshape(-1), atk.model(a4).reshape(-1)
    assert (torch.where(y == 1, z1 < z0, z1 > z0)).all() and ((a4 != x).sum(dim=1) <= 5).all()
