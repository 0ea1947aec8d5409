"""`-m gpu`: the perturbation report (include/advstep_perturb.h) against the float64 restatement tests/perturb_ref.py, through
the C ABI with canaries round its outputs, inside a captured graph, in the evaluation loop (flag on, flag off, two lanes) and
in the analyser's CSV.

The bounds on the re-associated sums are DERIVED from the kernel's summation order (csrc/perturb.hip), as
tests/test_gpu_momentum.py derives its own.  With u = 2^-24: a thread adds its 4 quads, each as (a + b) + (c + d), one after
the other (2 + 4 additions deep), a wave adds in 6 shuffle levels, the 4 waves in 3, the finishing launch adds
ceil(C / 256) partials per thread (C = ceil(T / 4096) tiles) and then 6 + 3 again: n = 24 + ceil(C / 256) additions on the
longest chain, and every term is non-negative.  To first order, relative to the float64 value,
    energy      (n + 1) u                 (the + 1: a square rounds once)
    l1_mean     (n + 1) u                 (|d| is exact; the + 1: the division by T)
    l2          ((n + 1) / 2 + 1) u       (half the relative error of sum d^2, and the square root rounds once)
and linf is exact.  In dB, with K = 10 / ln 10 = 4.343,
    snr_db      K (2 (n + 1) + 1) u + A   (two sums and their quotient)
    seg_snr_db  K (2 (8 + 1) + 1) u + A   per segment (a segment's sum is 2 + 6 additions deep; the clamp is 1-Lipschitz and the
                                          e_d == 0 decision is exact), + (n_s + 1) u mean|term| for the mean, n_s = 16 +
                                          ceil(C / 256): 4 terms per wave, the 4 waves in 3, then the finishing launch as above
A is the allowance for the device's log10f and the product by 10, which cannot be derived from the source.  Measured on the
MI355X over the rows of test_kernel_against_float64: snr_db never leaves the sum term there (its
largest deviation from float64 beyond K (2 (n + 1) + 1) u is negative, -1.2e-5 dB), so the log10f stage was taken alone — the
largest |snr_db - 10 log10(r)| in float64, r being the float32 quotient the kernel itself formed (its sums re-added on the
host in the kernel's order, bit for bit equal to the energy and l2 planes): 1.7e-6 dB, LOG10F_DB below.  A is four times
that: a few ulp of a value of up to about 120 dB, depending on the input.  Nothing else here was measured."""
import logging
import math

import numpy as np
import pytest
import torch

from tests import perturb_ref as R

pytestmark = pytest.mark.gpu

# (B, T, shift): the last one starts `shift` = 1 float off a 16-byte boundary
CASES = [(1, 1, 0), (3, 255, 0), (2, 256, 0), (5, 257, 0), (4, 4096, 0), (3, 4097, 0), (7, 8191, 0), (2, 64_600, 0), (3, 8192, 1)]
U = 2.0 ** -24
K_DB = 10.0 / math.log(10.0)
LOG10F_DB = 1.7e-6               # dB; measured on gfx950 (MI355X), see the module docstring and DESIGN.md section 4q
A_DB = 4 * LOG10F_DB
PAD = 1024                       # canary elements either side of an output (4096 bytes: keeps 16-byte alignment)
PLANTED = ("still", "silent", "both", "nan")
CFG = {"data": {"seed": 42}, "checkpoint": {"path": ""},
       "model": {"name": "lcnn", "parameters": {"frontend_algorithm": ["lfcc"], "input_channels": 1}}}


def hip():
    from audio_deepfake_adversarial_attacks_amd import hip_ops
    return hip_ops


def chain(T):
    return 24 + math.ceil(math.ceil(T / 4096) / 256)


def bounds(ref, x, d):
    """Absolute bound per plane and row, (6, B), from the float64 values `ref` = perturb_ref(x, d) (module docstring)."""
    B, T = x.shape
    n = chain(T)
    out = np.zeros((6, B))
    out[1] = (n + 1) * U * ref[1]
    out[2] = ((n + 1) / 2 + 1) * U * ref[2]
    out[3] = (n + 1) * U * ref[3]
    out[4] = K_DB * (2 * (n + 1) + 1) * U + A_DB
    if T // R.SEGMENT:
        n_s = 16 + math.ceil(math.ceil(T / 4096) / 256)
        out[5] = K_DB * 19 * U + A_DB + (n_s + 1) * U * np.abs(R.segment_terms(x, d)).mean(axis=1)
    return out


def check(got, x, adv, label):
    """got (6, B) float32 from the device against float64: the same NaNs and infinities, linf exact, the rest inside the bounds.
    Prints each plane's largest error / bound before asserting."""
    x, adv = np.asarray(x, dtype=np.float32), np.asarray(adv, dtype=np.float32)
    d = R.difference(x, adv)
    ref = R.perturb_ref(x, d)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    finite = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), label                  # NaN where the definition says NaN, only there
    assert np.array_equal(got[~finite & ~np.isnan(ref)], ref[~finite & ~np.isnan(ref)]), label     # +-inf exactly
    bound = bounds(ref, x, d)
    err = np.where(finite, np.abs(np.where(finite, got, 0.0) - np.where(finite, ref, 0.0)), 0.0)
    bound = np.where(finite, bound, 0.0)
    for k, name in enumerate(R.PLANES):
        print(f"  {label} {name}: max err {err[k].max():.3e}, max err / bound "
              f"{(err[k] / np.maximum(bound[k], 1e-300)).max() if k else 0.0:.3f}")
    assert np.array_equal(got[0][finite[0]], ref[0][finite[0]]), label          # linf: no rounding after d
    assert (err <= bound).all(), (label, np.argwhere(err > bound).tolist())
    return ref


def make_case(B, T, seed):
    """x ~ N(0, 0.05^2) clipped to [-1, 1]; d = N(0, 1) times a per-segment scale drawn log-uniformly over 1e-6 .. 1, so
    segments land below, inside and above the clamp range; then the planted rows, as many as B - 1 allows, their kinds taken
    in turn from `seed` on so that every kind meets several shapes.  Returns float32 (x, adv) and {row: kind}."""
    rng = np.random.default_rng(seed)
    x = np.clip(rng.normal(0.0, 0.05, (B, T)), -1, 1).astype(np.float32)
    scale = 10.0 ** rng.uniform(-6, 0, (B, -(-T // R.SEGMENT)))
    d = rng.normal(0.0, 1.0, (B, T)) * np.repeat(scale, R.SEGMENT, axis=1)[:, :T]
    adv = (x + d.astype(np.float32)).astype(np.float32)
    planted = {}
    for k in range(min(B - 1, len(PLANTED))):
        row, kind = B - 1 - k, PLANTED[(seed + k) % len(PLANTED)]
        planted[row] = kind
        if kind == "still":
            adv[row] = x[row]
        elif kind == "silent":
            adv[row] -= x[row]
            x[row] = 0.0
        elif kind == "both":
            x[row] = adv[row] = 0.0
        else:
            adv[row, T // 2] = np.nan
    return x, adv, planted


def padded(shape, fill, cuda, shift=0):
    n = int(np.prod(shape))
    buf = torch.full((PAD + shift + n + PAD,), fill, device=cuda)
    return buf, buf[PAD + shift:PAD + shift + n].view(shape)


def untouched(buf, fill, n, shift=0):
    return bool((buf[:PAD + shift] == fill).all() and (buf[PAD + shift + n:] == fill).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- the kernel ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,shift", CASES)
def test_kernel_against_float64(cuda, B, T, shift):
    """One sample; the first segment edge (255, 256, 257); the first tile edge (4096, 4097); T % 4 != 0 with unaligned later
    rows (255, 257, 4097, 8191); a base one float off a 16-byte boundary; the production row.  Through the C ABI with canaries
    round `stats` and the workspace, then through hip_ops on a side stream: bit-identical."""
    from audio_deepfake_adversarial_attacks_amd import _lib
    lib = _lib.load()
    x_h, adv_h, planted = make_case(B, T, seed=CASES.index((B, T, shift)))
    _, x = padded((B, T), 0.0, cuda, shift)
    _, adv = padded((B, T), 0.0, cuda, shift)
    x.copy_(torch.from_numpy(x_h)), adv.copy_(torch.from_numpy(adv_h))
    assert (x.data_ptr() % 16 != 0) == bool(shift)
    need = lib.advstep_perturb_stats_workspace_bytes(B, T)
    sbuf, stats = padded((6, B), 7.5, cuda)
    wbuf, ws = padded((need // 4,), -3.25, cuda)
    stream = torch.cuda.current_stream(cuda).cuda_stream
    assert lib.advstep_perturb_stats_f32(x.data_ptr(), adv.data_ptr(), stats.data_ptr(), ws.data_ptr(), need, B, T, stream) == 0
    torch.cuda.synchronize()
    assert untouched(sbuf, 7.5, 6 * B) and untouched(wbuf, -3.25, need // 4)
    assert not (stats == 7.5).any()                                             # every value written
    ref = check(stats.cpu().numpy(), x_h, adv_h, f"({B}, {T}, +{shift})")
    for row, kind in planted.items():                                           # the planted rows are what they were meant to be
        snr, seg = ref[4, row], ref[5, row]
        assert {"still": snr == np.inf and (seg == 35.0 or T < 256), "silent": snr == -np.inf and (seg == -10.0 or T < 256),
                "both": np.isnan(snr) and (seg == 35.0 or T < 256), "nan": np.isnan(snr) and np.isnan(ref[0, row])}[kind]
    random_rows = [r for r in range(B) if r not in planted]
    assert np.isfinite(ref[:5, random_rows]).all()                              # only planted rows may be NaN or infinite
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        again = hip().perturbation_stats(x, adv)
    side.synchronize()
    assert again.shape == (6, B) and torch.equal(bits(again), bits(stats))
    assert torch.equal(bits(hip().perturbation_stats(x, adv, out=torch.empty_like(again))), bits(stats))


def test_empty_batches(cuda):
    """T == 0 writes the empty-row values without reading anything; B == 0 launches nothing."""
    got = hip().perturbation_stats(torch.empty(3, 0, device=cuda), torch.empty(3, 0, device=cuda)).cpu().numpy()
    assert got[[0, 2, 3]].tolist() == [[0.0] * 3] * 3 and np.isnan(got[[1, 4, 5]]).all()
    assert hip().perturbation_stats(torch.empty(0, 9, device=cuda), torch.empty(0, 9, device=cuda)).shape == (6, 0)
    with pytest.raises(ValueError):
        hip().perturbation_stats(torch.zeros(2, 8, device=cuda), torch.zeros(2, 9, device=cuda))


# ---- known answer, inside a captured graph ----------------------------------------------------------------------------------

def test_fgsm_linf_is_eps_inside_a_captured_graph(cuda):
    """FGSM moves every sample of a [0, 1] batch by eps or, at the box, by less: linf in the min-max domain is eps up to the
    rounding of x + eps s (half a spacing of [0.5, 1): 2^-25) and of the difference.  The report is captured into a graph and
    replayed; the replay equals the eager call bit for bit."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import synthetic_waveforms
    from tests.test_gpu_apgd import detector
    eps = 0.001
    model = detector("lcnn", cuda)
    x, y = synthetic_waveforms(4, seed=7)
    x01, _, _ = hip().to_minmax(x.to(cuda))
    atk = torchattacks.FGSM(model, eps=eps)
    atk.set_training_mode(model_training=True, batchnorm_training=False)
    adv01 = atk(x01, y.to(cuda)).contiguous()
    eager = hip().perturbation_stats(x01, adv01)
    out = torch.full((6, 4), -1.0, device=cuda)
    stream, graph = torch.cuda.Stream(cuda), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        hip().perturbation_stats(x01, adv01, out=out)
    owned = hip().release_stream_workspaces(stream.cuda_stream)       # the graph writes to this workspace on every replay
    assert len(owned) >= 1
    out.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(eager))
    check(out.cpu().numpy(), x01.cpu().numpy(), adv01.cpu().numpy(), "fgsm")
    linf, l1_mean, l2 = (out[k].cpu().numpy().astype(np.float64) for k in (0, 1, 2))
    assert (linf <= (eps + 2.0 ** -25) * (1 + U)).all() and (linf >= eps - 2.0 ** -24).all()
    assert (l1_mean <= linf).all() and (l2 <= linf * math.sqrt(x01.shape[1]) * (1 + 30 * U)).all()
    assert np.isfinite(out.cpu().numpy()).all()


# ---- the evaluation loop -----------------------------------------------------------------------------------------------------

class Collect(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def run_loop(cuda, pairs=None, **kw):
    """FGSM on LCNN + LFCC over 16 synthetic utterances in 4 batches -> (report, the INFO lines the run logged)."""
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks

    def keep(batch_x, batch_x_attacked, **_):
        pairs.append((batch_x.cpu().numpy(), batch_x_attacked.cpu().numpy()))

    torch.manual_seed(5)
    log, level = Collect(), logging.getLogger().level
    logging.getLogger().addHandler(log)
    logging.getLogger().setLevel(logging.INFO)
    try:
        report = generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=torchattacks.FGSM,
                                  attack_params={"eps": 0.001}, batch_size=4, dataset=SyntheticDetectionDataset(16),
                                  share_weights=True, shuffle=False, num_workers=0, return_scores=True,
                                  on_attack_end_callback=keep if pairs is not None else None, **kw)
    finally:
        logging.getLogger().removeHandler(log)
        logging.getLogger().setLevel(level)
    return report, log.lines


@pytest.fixture(scope="module")
def loop_with_flag(cuda):
    pairs = []
    report, lines = run_loop(cuda, pairs, perturbation_stats=True)
    return report, pairs, lines


def test_loop_reports_the_perturbation_of_its_own_batches(loop_with_flag):
    from audio_deepfake_adversarial_attacks_amd import metrics
    report, pairs, lines = loop_with_flag
    assert len(pairs) == 4
    x, adv = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    planes = report["scores"]["perturbation"]
    assert list(planes) == list(R.PLANES) and all(v.shape == (16,) and v.dtype == np.float32 for v in planes.values())
    check(np.stack([planes[k] for k in R.PLANES]), x, adv, "loop")                          # per utterance, in order
    scores = report["scores"]
    want = metrics.perturbation_summary(planes, scores["y_pred_label"] != scores["y"])
    assert len(want) == 17
    for k, v in want.items():
        assert report[k] == v or (np.isnan(v) and np.isnan(report[k])), k
    assert report["perturbation/nan_rows"] == 0 and 0 < report["perturbation/linf_max"] < 1  # waveform domain: eps (max - min)
    at = [i for i, m in enumerate(lines) if m.startswith("adv_eval/eer")]                   # the second log line
    assert len(at) == 1 and lines[at[0] + 1].startswith("perturbation/linf_max: ") and "nan_rows: 0" in lines[at[0] + 1]
    assert "misclassified" not in lines[at[0] + 1]


def test_loop_without_the_flag_is_the_old_report(cuda, loop_with_flag):
    off, lines = run_loop(cuda)
    assert lines[-1].startswith("adv_eval/eer") and not any("perturbation" in m for m in lines)
    assert set(off) == {f"adv_eval/{k}" for k in ("eer", "accuracy", "precision", "recall", "f1_score", "auc")} | \
        {"num_total", "scores"}
    assert set(off["scores"]) == {"y_pred", "y_pred_label", "y"}
    on = loop_with_flag[0]
    for k in off:                                                                # and the flag changes nothing it shares
        if k != "scores":
            assert off[k] == on[k], k
    assert all(np.array_equal(off["scores"][k], on["scores"][k]) for k in off["scores"])


@pytest.fixture
def fresh_graphs():
    from audio_deepfake_adversarial_attacks_amd.torchattacks import graphed
    graphed.clear()
    yield graphed
    graphed.clear()


def test_two_batches_in_flight_give_the_same_planes(cuda, fresh_graphs):
    from audio_deepfake_adversarial_attacks_amd import torchattacks
    from audio_deepfake_adversarial_attacks_amd.datasets.synthetic import SyntheticDetectionDataset
    from audio_deepfake_adversarial_attacks_amd.evaluation import generate_attacks

    def evaluate(in_flight):
        torch.manual_seed(5)                             # the random starts' Philox keys come from the global generator
        fresh_graphs.clear()
        return generate_attacks([None, None, None], CFG, str(cuda), attack_model_config=CFG, attack_method=torchattacks.PGD,
                                attack_params={"eps": 0.003, "steps": 4}, batch_size=4, dataset=SyntheticDetectionDataset(32),
                                share_weights=True, shuffle=False, num_workers=0, return_scores=True, in_flight=in_flight,
                                perturbation_stats=True)

    one, two = evaluate(1), evaluate(2)
    for k in R.PLANES:
        a, b = one["scores"]["perturbation"][k], two["scores"]["perturbation"][k]
        assert a.shape == (32,) and np.array_equal(a.view(np.int32), b.view(np.int32)), k
    assert np.isfinite(one["scores"]["perturbation"]["snr_db"]).all()
    assert all(one[k] == two[k] for k in one if k.startswith("perturbation/") and not np.isnan(one[k]))


# ---- the analyser's CSV --------------------------------------------------------------------------------------------------------

def test_analyser_writes_one_csv_line_per_wav_pair(cuda, tmp_path, capsys):
    from audio_deepfake_adversarial_attacks_amd.aa.qualitative.attacks_analysis import AttackAnalyser
    from audio_deepfake_adversarial_attacks_amd.datasets import audio_io
    B, T = 6, 1000
    rng = np.random.default_rng(4)
    x_h = np.clip(rng.normal(0.0, 0.05, (B, T)), -1, 1).astype(np.float32)
    adv_h = (x_h + (rng.normal(0.0, 1.0, (B, T)) * 10.0 ** rng.uniform(-4, -1, (B, 1))).astype(np.float32)).astype(np.float32)
    y = torch.tensor([1, 1, 0, 0, 1, 0])
    clean = y.to(torch.int32)
    attacked = torch.tensor([0, 1, 1, 0, 1, 1], dtype=torch.int32)              # rows 0 (fn), 2 and 5 (fp) flipped
    meta = [["melgan"] * B, [f"/data/corpus/utt{i}.wav" for i in range(B)], ["val"] * B, torch.full((B,), 4.0)]

    def analyse(dst, **kw):
        AttackAnalyser(dst, **kw).analyse(
            batch_x=torch.from_numpy(x_h).to(cuda), batch_x_attacked=torch.from_numpy(adv_h).to(cuda), batch_y=y.to(cuda),
            batch_preds_label=attacked.to(cuda), batch_preds=torch.rand(B, device=cuda),
            batch_preds_noattack_label=clean.to(cuda), batch_preds_noattack=torch.rand(B, device=cuda), batch_metadata=meta)

    analyse(tmp_path / "off")
    assert not (tmp_path / "off" / "perturbation_metrics.csv").exists()          # default: the folder of before
    analyse(tmp_path / "on", stats_csv=True)
    analyse(tmp_path / "on", stats_csv=True)                                     # a second batch appends, no second header
    capsys.readouterr()
    lines = (tmp_path / "on" / "perturbation_metrics.csv").read_text().splitlines()
    assert lines[0] == "name,kind,linf,l1_mean,l2,snr_db,seg_snr_db" and len(lines) == 1 + 2 * 3 and lines[1:4] == lines[4:]
    wavs = sorted(p.name for p in (tmp_path / "on").glob("*.wav"))
    assert len(wavs) == 2 * 3 and wavs == sorted(p.name for p in (tmp_path / "off").iterdir())
    assert [ln.split(",")[1] for ln in lines[1:4]] == ["fp", "fp", "fn"]
    for ln in lines[1:4]:
        name, kind, *values = ln.split(",")
        orig, _ = audio_io.load(tmp_path / "on" / f"{name}_{kind}_original.wav")
        atkd, _ = audio_io.load(tmp_path / "on" / f"{name}_{kind}_attacked.wav")
        got = np.array([float(v) for v in values], dtype=np.float32)
        got = np.insert(got, 3, (orig.double() ** 2).sum().item())              # the CSV has no energy column
        check(got.reshape(6, 1), orig.numpy(), atkd.numpy(), name)
