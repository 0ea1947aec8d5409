"""The adversarial-evaluation loop (reference: evaluate_models_on_adversarial_attacks.py:146-298).

`generate_attacks` keeps the reference's signature and per-batch order of operations
(min-max -> attack -> revert -> target forward -> sigmoid / threshold -> accumulate -> final report) and its
log line.  What is different is how the work is placed on the machine:

  * one process per GPU instead of `nn.DataParallel` (reference :163,:167): every rank owns a replica of both
    models and a CONTIGUOUS slice of each global batch — the same chunking DataParallel's scatter would do, so
    the LFCC batch-wide dB floor sees the same rows — and there is NO per-step traffic between GPUs;
  * batches reach the device one batch ahead of the attack, through pinned staging buffers on a side stream
    (`_device_batches`): the reference's blocking `.to(device)` per batch would idle the GPU for a copy + collation;
  * scores stay on the device until the end (the reference synchronises with `.item()` / `.cpu()` every batch,
    :261-265); one D2H copy per run;
  * the final aggregate is the only communication: an all-reduce(SUM) of the two counters and one all-gather of
    the packed (score, predicted label, label) rows over RCCL/xGMI (`backend="nccl"`), or gloo on CPU tests
    Every optional report of the run (`_active_reports`) adds at most one exchange of its own behind them, in the reports'
    order: a per-utterance report (`_RowReport`) one all-gather of its rows, a MultiAttack one all-reduce of its survivor
    counts, `channel=` one all-reduce of its five counters, `certify=` one all-gather per dtype of its rows (two), a universal
    attack none.
"""
from __future__ import annotations

import logging
import contextlib
import functools
import os
from types import SimpleNamespace
from typing import Any, Callable, Dict, Iterator, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, Dataset, Sampler

from . import metrics
from .aa import utils as aa_utils
from .datasets.base_dataset import WAVE_FAKE_CUT, SimpleAudioFakeDataset, ragged_collate
from .datasets.detection_dataset import DetectionDataset
from .datasets.synthetic import SyntheticDetectionDataset
from .datasets.wave_ops import RaggedWaveBatch
from .utils import load_model

LOGGER = logging.getLogger()


# ---------------------------------------------------------------------------------------------------------
# ranks and shards
# ---------------------------------------------------------------------------------------------------------

def rank_and_world() -> Tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def shard_bounds(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous [lo, hi) of rank `rank` when n rows are cut into `world` chunks (torch.chunk / DataParallel
    scatter semantics: every chunk has ceil(n / world) rows except possibly the last ones)."""
    per = -(-n // world)
    lo = min(rank * per, n)
    return lo, min(lo + per, n)


class ShardedBatchSampler(Sampler[List[int]]):
    """Yields, for every GLOBAL batch (drop_last=True as in the reference's DataLoader, :197-203), the indices
    of this rank's contiguous slice.  The permutation comes from a dedicated generator seeded identically on
    every rank, so all ranks agree on the global batches without communicating."""

    def __init__(self, n_items: int, global_batch: int, rank: int = 0, world: int = 1, shuffle: bool = True,
                 seed: int = 42):
        if global_batch % world != 0:
            raise ValueError(f"global batch {global_batch} is not divisible by world size {world}")
        self.n_items, self.global_batch, self.rank, self.world = n_items, global_batch, rank, world
        self.shuffle, self.seed = shuffle, seed

    def __len__(self) -> int:
        return self.n_items // self.global_batch

    def __iter__(self) -> Iterator[List[int]]:
        if self.shuffle:
            order = torch.randperm(self.n_items, generator=torch.Generator().manual_seed(self.seed)).tolist()
        else:
            order = list(range(self.n_items))
        lo, hi = shard_bounds(self.global_batch, self.rank, self.world)
        for b in range(len(self)):
            batch = order[b * self.global_batch:(b + 1) * self.global_batch]
            yield batch[lo:hi]


def aggregate_across_ranks(y_pred: torch.Tensor, y_pred_label: torch.Tensor, y: torch.Tensor,
                           num_correct: torch.Tensor, num_total: torch.Tensor):
    """End-of-run exchange.  Inputs are this rank's 1-D tensors / 0-d counters on the
    compute device; returns numpy arrays for the whole job, ordered by rank, plus the two global counters."""
    rank, world = rank_and_world()
    packed = torch.stack([y_pred.float(), y_pred_label.float(), y.float()], dim=1).contiguous()  # (n_local, 3)
    counters = torch.stack([num_correct.to(torch.int64), num_total.to(torch.int64)])
    if world > 1:
        dist.all_reduce(counters, op=dist.ReduceOp.SUM)
        parts = [torch.empty_like(packed) for _ in range(world)]
        dist.all_gather(parts, packed)
        packed = torch.cat(parts, dim=0)
    host = packed.cpu().numpy()
    c = counters.cpu().numpy()
    return host[:, 0].astype(np.float32), host[:, 1].astype(np.int32), host[:, 2].astype(np.int64), int(c[0]), int(c[1])


def gather_rows_across_ranks(rows: torch.Tensor) -> np.ndarray:
    """This rank's (n_local, k) per-utterance rows on the compute device -> the whole job's (N, k) numpy array, ordered by
    rank like the arrays of `aggregate_across_ranks` (one all-gather; every rank holds the same n_local: drop_last=True)."""
    rows = rows.contiguous()
    if rank_and_world()[1] > 1:
        parts = [torch.empty_like(rows) for _ in range(rank_and_world()[1])]
        dist.all_gather(parts, rows)
        rows = torch.cat(parts, dim=0)
    return rows.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------
# per-batch body
# ---------------------------------------------------------------------------------------------------------

def attack_batch(atk, batch_x: torch.Tensor, batch_y: torch.Tensor) -> torch.Tensor:
    """Reference :218-221 — normalise each utterance to [0, 1], attack, map back to the original range."""
    x01, mn, mx = aa_utils.to_minmax(batch_x)
    if getattr(atk, "wants_minmax", False):                # a budget stated in the waveform's domain (torchattacks.PGDSNR)
        atk.set_minmax(mn, mx)
    adv01 = atk(x01, batch_y)
    return aa_utils.revert_minmax(adv01, mn, mx)


@torch.no_grad()
def score_batch(model, batch_x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reference :236-238 — probability of the bonafide class and the hard label ((p + .5).int() == p >= .5)."""
    preds = torch.sigmoid(model(batch_x).squeeze(1).detach())
    return preds, (preds + 0.5).int()


def format_report(report: Dict[str, float]) -> str:
    """The reference's final log line (:295-298)."""
    order = ("eer", "accuracy", "precision", "recall", "f1_score", "auc")
    return ", ".join(f"adv_eval/{k}: {report['adv_eval/' + k]:.4f}" for k in order)


def format_keys(report: Dict[str, float], prefix: str, integer_suffixes=(), float_spec: str = ".4g", exclude: Optional[str] = None) -> str:
    """The log line of one optional report: the report's `prefix/` keys in their order (without those under `exclude`), a value
    whose key ends in one of `integer_suffixes` as it is (a count), every other one with `float_spec`."""
    keys = [k for k in report if k.startswith(prefix + "/") and not (exclude and k.startswith(exclude))]
    return ", ".join(f"{k}: {report[k]}" if k.endswith(integer_suffixes) else f"{k}: {report[k]:{float_spec}}" for k in keys)


# the public names of the optional reports' log lines (metrics.*_summary says what the keys mean)
format_perturbation = functools.partial(format_keys, prefix="perturbation", integer_suffixes="nan_rows",
                                        exclude="perturbation/misclassified/")
format_min_radius = functools.partial(format_keys, prefix="min_radius")
format_universal = functools.partial(format_keys, prefix="universal", integer_suffixes="_utterances")
format_filter = functools.partial(format_keys, prefix="filter", integer_suffixes="/taps")
format_blackbox = functools.partial(format_keys, prefix="blackbox", integer_suffixes="budget")
format_sparse = functools.partial(format_keys, prefix="sparse", integer_suffixes=("_max", "/k"))
format_masking = functools.partial(format_keys, prefix="masking")
format_channel = functools.partial(format_keys, prefix="channel", integer_suffixes=("draws", "flipped"), float_spec=".4f")
format_certified = functools.partial(format_keys, prefix="certified", integer_suffixes=("/n", "violations"))


# ---------------------------------------------------------------------------------------------------------
# optional reports
# ---------------------------------------------------------------------------------------------------------

class _Report:
    """One optional report of a run; everything the loop does for it is here.  `generate_attacks` asks `_active_reports` once
    which ones a run has and from then on only walks that list, in the order of the report's keys and of the log lines:
      batch(atk, clean, attacked)    after the attack (or the copy of a run without one), under the lane's stream, on the loop's
                                     waveform-domain tensors; returns the tensors it produced there, which the loop hands to
                                     `lanes.keep`: the caller's stream reads them after join()
      scored(lane, model, ...)       after the detector has scored the attacked batch; returns the same
      finish(ctx)                    after the lanes have joined: the report's keys, in order, and whatever it communicates.  `ctx`:
                                     all_y, all_label (the whole job's numpy arrays), samples (of an utterance), rank, world, device
      scores()                       after finish: its entries of report["scores"] (`return_scores`)
      line(report)                   its log line; `leads`: ahead of the reference's line, not behind it"""
    leads = False

    def batch(self, atk, clean, attacked):
        return ()

    def scored(self, lane, model, clean, attacked, labels, attacked_label, post):
        return ()

    def scores(self) -> Dict[str, Any]:
        return {}


class _RowReport(_Report):
    """A per-utterance report.  `source(atk, clean, attacked)` gives a batch's rows, (B,) or (B, width) on the device, without a
    host read; at the end ONE all-gather brings the job's rows to the host, in utterance order like `y_pred` and as `dtype`
    (`names`: as a dict of the named columns), `summary(rows, ctx)` turns them into the report's keys, `scores()` returns them
    under `key` and `line` is the report's `format_*`."""

    def __init__(self, key: str, source, dtype, summary, line, width: int = 1, names=None):
        self.key, self.source, self.dtype, self.summary, self.line, self.width, self.names = key, source, dtype, summary, line, width, names
        self.parts: List[torch.Tensor] = []

    def batch(self, atk, clean, attacked):
        self.parts.append(self.source(atk, clean, attacked))
        return self.parts[-1:]

    def finish(self, ctx):
        rows = gather_rows_across_ranks(torch.cat(self.parts).reshape(-1, self.width))
        self.rows = np.ascontiguousarray(rows[:, 0] if self.width == 1 else rows, dtype=self.dtype)
        if self.names:
            self.rows = {name: np.ascontiguousarray(self.rows[:, k]) for k, name in enumerate(self.names)}
        return self.summary(self.rows, ctx)

    def scores(self):
        return {self.key: self.rows}


def masking_pass(masking, batch_x: torch.Tensor, batch_x_attacked: torch.Tensor) -> torch.Tensor:
    """(B, 3) masking statistics of what the attack did to a batch, any attack's or none's: both waveforms are mapped to the
    attack's domain with the CLEAN utterance's minimum and maximum (the same arithmetic for both, so untouched samples give an
    exact 0), then `masking.threshold` of the clean one and one `hip_ops.masking_hinge_grad` launch.  No host read."""
    from . import hip_ops
    B = batch_x.shape[0]
    x, adv = batch_x.reshape(B, -1), batch_x_attacked.reshape(B, -1)
    mn, mx = x.amin(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)
    span = (mx - mn).clamp_min(torch.finfo(torch.float32).tiny)
    x01, adv01 = ((x - mn) / span).contiguous(), ((adv - mn) / span).contiguous()
    theta, scale = masking.threshold(x01, hip_ops)
    return hip_ops.masking_hinge_grad(adv01, x01, masking.window(x.device), theta, scale, masking.hop)[1]


class _UniversalReport(_Report):
    """A universal attack (`is_universal`: torchattacks.UniversalPGD) gets its perturbation BEFORE the loop (`prepare_universal`,
    when this object is made: on the caller's stream, before the lanes exist): loaded from `load`, or fitted on the first `fit`
    batches of this run's batch order (None: a quarter of them, at least 1), which are kept on the device meanwhile
    (fit x B x T x 4 bytes); `save` writes it.  The loop then runs over ALL batches with the frozen perturbation, one launch per
    batch.  More than one rank needs `load`; no communication either way.  Adds the `universal/*` keys of
    `metrics.universal_summary` (fitted against held-out utterances) and `scores["universal_delta"]`."""

    line = staticmethod(format_universal)

    def __init__(self, atk, loader, device, n_batches: int, fit, load, save):
        self.atk = atk
        self.fitted_rows = prepare_universal(atk, loader, device, n_batches, fit, load, save)

    def finish(self, ctx):
        self.delta = self.atk.delta.detach().cpu().numpy()
        # rank order = utterance order for the one process that fits; a loaded perturbation was fitted on none of them
        return metrics.universal_summary(ctx.all_y, ctx.all_label, np.arange(len(ctx.all_y)) < self.fitted_rows, self.delta,
                                         self.atk.source_label)

    def scores(self):
        return {"universal_delta": self.delta}


class _FilterReport(_UniversalReport):
    """A universal FILTER (`is_filter`: torchattacks.UniversalFilter) goes through the same protocol; what it carries is taps, not
    an additive perturbation, so the report keeps `universal_summary`'s group keys (sizes, accuracy_*, source_flipped_*), drops
    its two `delta_*` norms and adds the `filter/*` keys of `metrics.filter_summary`; `scores["universal_delta"]` holds the taps."""

    @staticmethod
    def line(report):
        return ", ".join(filter(None, (format_universal(report), format_filter(report))))

    def finish(self, ctx):
        out = super().finish(ctx)
        for key in ("universal/delta_linf", "universal/delta_l2"):
            del out[key]
        out.update(metrics.filter_summary(self.delta))
        return out


class _MultiAttackReport(_Report):
    """A MultiAttack reports the utterances left after every member as well (multiattack.py's `save` mechanism: accumulate the
    records of every call): `multi_attack/remaining`, summed over the ranks by one all-reduce of (n_members + 1) int64, and the
    MultiAttack's own record line, ahead of the reference's."""

    leads = True

    def __init__(self, atk):
        self.atk = atk
        atk._start_multi_atk_records()

    def finish(self, ctx):
        remaining = torch.tensor([int(r) for r in self.atk._multi_atk_records], dtype=torch.int64, device=ctx.device)
        self.atk._clear_multi_atk_records()
        self.atk._accumulate_multi_atk_records = False
        if ctx.world > 1:
            dist.all_reduce(remaining, op=dist.ReduceOp.SUM)
        return {"multi_attack/remaining": remaining.tolist()}

    def line(self, report):
        return self.atk._return_sr_record(report["multi_attack/remaining"])


class _ChannelScorer(_Report):
    """`channel=` (a torchattacks.Channel or the name of a preset in torchattacks.CHANNELS): what is left of the attack — any
    attack, or none — after a simulated audio channel, counted on the device.  Per batch: N draws of the channel, the
    SAME draws and noise for the attacked and the clean waveform (a paired comparison), in the waveform's domain (centre 0); the
    detector scores each draw's B rows under no_grad, like every other forward of the loop.  Five counters: (utterance, draw)
    pairs, attacked pairs judged right, clean pairs judged right, pairs of utterances the attack flipped without the channel
    (clean judged right, attacked judged wrong, both unchannelled), and those of them still judged wrong through it.
    The draws and the noise seeds come from generators of the scorer's own (seeded with `seed`), so the attack sees the random
    numbers it would see in a run without `channel=`.  Adds `channel/accuracy` (per cent, over all pairs, like
    adv_eval/accuracy), `channel/clean_accuracy`, `channel/survival` (the share of pairs still misclassified among the utterances
    the attack flipped without the channel; 0 when it flipped none: `channel/flipped` says how many) and, over several ranks,
    one all-reduce of the five counters.  `adv_eval/*` and every other key are computed exactly as without it, from the
    unchannelled waveform."""

    line = staticmethod(format_channel)

    def __init__(self, channel, draws: int, device, seed: int = 0):
        from . import hip_ops
        from .torchattacks.channel import resolve
        self.ops, self.channel, self.draws = hip_ops, resolve(channel), int(draws)
        if not 1 <= self.draws <= hip_ops.CHANNEL_MAX_DRAWS:
            raise ValueError(f"channel_draws must lie between 1 and {hip_ops.CHANNEL_MAX_DRAWS}, got {draws}")
        self.device = device
        self.host_gen = torch.Generator().manual_seed(seed)
        self.device_gen = torch.Generator(device=device).manual_seed(seed)
        self.pairs = 0                                  # counted on the host: B per draw
        self.counters: Dict[int, torch.Tensor] = {}     # lane -> the other four, int64 on the device

    def scored(self, lane, model, clean, attacked, labels, attacked_label, post):
        """`post`: the loop's preprocessing between the waveform and the detector (raw_sample_from_dataset), or None."""
        ops, N = self.ops, self.draws
        c = self.counters.setdefault(lane, torch.zeros(4, dtype=torch.int64, device=self.device))
        y = labels.int()
        zero = torch.zeros(clean.shape[0], dtype=torch.float32, device=clean.device)
        params = self.channel.draw(N, clean, zero, generator=self.device_gen)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=self.host_gen).item())   # on the host: no device sync
        through_adv = ops.channel_apply(attacked.contiguous(), zero, *params, seed=seed)
        through_clean = ops.channel_apply(clean.contiguous(), zero, *params, seed=seed)
        score = (lambda x: score_batch(model, post(x))[1]) if post is not None else (lambda x: score_batch(model, x)[1])
        flipped = (score(clean) == y) & (attacked_label != y)
        for j in range(N):
            adv_right, clean_right = score(through_adv[j]) == y, score(through_clean[j]) == y
            c += torch.stack([adv_right.sum(), clean_right.sum(), flipped.sum(), (flipped & ~adv_right).sum()])
        self.pairs += N * y.numel()
        return ()                                       # the counters live as long as the scorer

    def finish(self, ctx):
        total = torch.stack(list(self.counters.values())).sum(dim=0)
        total = torch.cat([torch.tensor([self.pairs], dtype=torch.int64, device=total.device), total])
        if ctx.world > 1:
            dist.all_reduce(total, op=dist.ReduceOp.SUM)
        pairs, adv_right, clean_right, flipped, still = (int(v) for v in total.cpu().tolist())
        return {"channel/accuracy": (adv_right / pairs) * 100, "channel/clean_accuracy": (clean_right / pairs) * 100,
                "channel/survival": still / flipped if flipped else 0.0, "channel/flipped": flipped // self.draws,
                "channel/draws": self.draws}


class _CertifyScorer(_Report):
    """`certify=sigma`: randomized smoothing's certificate (Cohen, Rosenfeld and Kolter, ICML 2019) of the detector on the CLEAN
    waveform of every batch — Cohen's protocol, whatever the attack, or none — through `torchattacks.Smoothing`: `n0` noisy
    copies pick a class, `n` fresh ones give its count kA, and at the end of the run `metrics.certified_summary` turns the counts
    into radii (host-side float64) and the `certified/*` keys.  `sigma` and the radii are in the WAVEFORM's units, one noise
    level for every utterance; the normalised figures divide by the clean utterance's max - min, the unit of every `eps` of
    AttackEnum (exact for the loop's threat model: the attack's waveform perturbation is span * delta).

    With an attack (`attacked`), PREDICT also votes on the attacked waveform with `n0` copies:
      certified/attacked_accuracy    per cent of utterances the smoothed detector still gets right (not abstained, right class)
      certified/attacked_abstained   per cent on which PREDICT abstains (metrics.smoothed_prediction)
      certified/violations           utterances where the attack's waveform-domain L2 (hip_ops.perturbation_stats) is BELOW the
                                     certified radius, neither procedure abstained and PREDICT gives the other class: 0 with
                                     probability >= 1 - alpha per utterance when the implementation is sound
    Every vote's noise is keyed by (seed, offset): a host counter advances by the slots a batch used, so the offsets follow the
    loop's batch order whatever the lanes do, and rank r starts at r << 40.  Per batch the scorer keeps an int32 and a float32
    row block on the device; `finish` makes one all-gather per dtype.  No host read before that.  The forwards are no_grad and
    come after the batch was scored: `adv_eval/*` and every other key are computed exactly as without it.  The frontends'
    dB floor is batch-wide, so a copy's logit depends on the rows forwarded with it: what is certified is the detector with
    that floor as these chunks form it (SPSA and HopSkipJump query it the same way)."""

    line = staticmethod(format_certified)

    def __init__(self, sigma: float, samples: int, select: int, alpha: float, device, seed: int = 0, rank: int = 0,
                 attacked: bool = False, report_at=metrics.CERTIFIED_REPORT_AT):
        from . import hip_ops
        from .torchattacks import Smoothing
        self.ops, self.device, self.attacked, self.report_at = hip_ops, device, bool(attacked), tuple(report_at)
        self.smooth = Smoothing(sigma, n=samples, n0=select, alpha=alpha, seed=seed)    # raises on a bad sigma, n, n0 or alpha
        self.offset = int(rank) << 40
        self.int_rows: List[torch.Tensor] = []          # per batch, in the loop's order: (B, 3) int32
        self.float_rows: List[torch.Tensor] = []        # (B, 2) float32

    def scored(self, lane, model, clean, attacked, labels, attacked_label, post):
        sm, B = self.smooth, clean.shape[0]
        cert = sm.certify(model, clean, self.offset, post)
        self.offset += sm.slots_certify
        flat = clean.reshape(B, -1)
        span = flat.amax(dim=1) - flat.amin(dim=1)
        if self.attacked:
            c1 = sm.predict(model, attacked, self.offset, post)[:, 0]
            self.offset += sm.slots_predict
            l2 = self.ops.perturbation_stats(clean.contiguous(), attacked.contiguous())[metrics.PERTURBATION_PLANES.index("l2")]
        else:
            c1, l2 = torch.zeros_like(cert[:, 0]), torch.zeros_like(span)
        self.int_rows.append(torch.cat([cert, c1.unsqueeze(1)], dim=1))
        self.float_rows.append(torch.stack([span, l2], dim=1))
        return self.int_rows[-1], self.float_rows[-1]

    def finish(self, ctx):
        sm = self.smooth
        ints = gather_rows_across_ranks(torch.cat(self.int_rows)).astype(np.int64)
        floats = gather_rows_across_ranks(torch.cat(self.float_rows)).astype(np.float64)
        y = np.asarray(ctx.all_y, dtype=np.int64).ravel()
        radius = np.asarray(metrics.certified_radius(ints[:, 1], sm.n, sm.alpha, sm.sigma), dtype=np.float64).reshape(-1)
        self.rows = {"class": ints[:, 0].astype(np.int32), "kA": ints[:, 1].astype(np.int32), "radius": radius,
                     "span": floats[:, 0].astype(np.float32)}
        out = metrics.certified_summary(ints[:, :2], y, floats[:, 0], sm.sigma, sm.n, sm.n0, sm.alpha, self.report_at)
        if self.attacked:
            pred = np.asarray(metrics.smoothed_prediction(ints[:, 2], sm.n0, sm.alpha), dtype=np.int64).reshape(-1)
            l2 = floats[:, 1]
            out["certified/attacked_accuracy"] = 100.0 * float(np.mean(pred == y)) if y.size else float("nan")
            out["certified/attacked_abstained"] = 100.0 * float(np.mean(pred < 0)) if y.size else float("nan")
            out["certified/violations"] = int(np.sum((radius >= 0.0) & (l2 < radius) & (pred >= 0) & (pred != ints[:, 0])))
            self.rows.update({"attacked_c1": ints[:, 2].astype(np.int32), "attacked_class": pred.astype(np.int32),
                              "l2": l2.astype(np.float32)})
        return out

    def scores(self):
        return {"certified": self.rows}


def _active_reports(atk, device, seed: int, loader, n_batches: int, perturbation_stats: bool, masking_stats: bool, channel,
                    channel_draws: int, universal_fit, universal_load, universal_save, certify=None, certify_samples: int = 1000,
                    certify_select: int = 100, certify_alpha: float = 0.001) -> List[_Report]:
    """The optional reports of a run, in the order of their keys and log lines; the one place that names them.  An attack-borne
    report is active when the attack HAS the attribute before its first call (None until then).  A run with every keyword off
    and an attack that carries nothing gets an empty list: the loop does nothing for them."""
    from .torchattacks import MaskingModel, MultiAttack

    def carries(name):
        return atk is not None and hasattr(atk, name)

    reports: List[_Report] = []
    if perturbation_stats:
        # one more row pass per batch over the batch and what the detector is given after `revert_minmax`, so the min-max round
        # trip's rounding of samples the attack did not move is part of the figure; six (B,) planes
        from . import hip_ops
        reports.append(_RowReport("perturbation", lambda atk, clean, attacked: hip_ops.perturbation_stats(clean, attacked).t(),
                                  np.float32, lambda planes, ctx: metrics.perturbation_summary(planes, ctx.all_label != ctx.all_y),
                                  format_perturbation, width=len(metrics.PERTURBATION_PLANES), names=metrics.PERTURBATION_PLANES))
    if carries("last_radius"):      # MinRadiusPGD: each utterance's minimal radius; HopSkipJump: the one a label-only attacker reached
        reports.append(_RowReport("min_radius", lambda atk, clean, attacked: atk.last_radius, np.float32,
                                  lambda rows, ctx: metrics.radius_summary(rows, getattr(atk, "report_at", ())), format_min_radius))
    if carries("last_queries"):     # SPSA, HopSkipJump: the model queries each utterance spent, against the attack's budget
        reports.append(_RowReport("queries", lambda atk, clean, attacked: atk.last_queries, np.int32,
                                  lambda rows, ctx: metrics.query_summary(rows, atk.budget), format_blackbox))
    if carries("last_changed"):     # PGDL0: the samples of each utterance it changed, against the attack's k
        reports.append(_RowReport("changed", lambda atk, clean, attacked: atk.last_changed, np.int64,
                                  lambda rows, ctx: metrics.sparsity_summary(rows, atk.k), format_sparse))
    if masking_stats or carries("last_masking"):
        # PsyPGD: the (B, 3) masking statistics of the rows it returned.  `masking_stats`: those of ANY attack, or none, and in
        # place of the attack's own: `masking_pass` rates the batch against the clean utterance's masking threshold (hop 128 or
        # the attack's own) in the attack's domain, one threshold and one launch per batch.  257 cells per frame
        masking = getattr(atk, "masking", None) or MaskingModel()
        reports.append(_RowReport("masking", (lambda atk, clean, attacked: masking_pass(masking, clean, attacked)) if masking_stats
                                  else (lambda atk, clean, attacked: atk.last_masking), np.float32,
                                  lambda rows, ctx: metrics.masking_summary(rows, masking.frames(ctx.samples) * 257),
                                  format_masking, width=3))
    if getattr(atk, "is_universal", False):
        kind = _FilterReport if getattr(atk, "is_filter", False) else _UniversalReport
        reports.append(kind(atk, loader, device, n_batches, universal_fit, universal_load, universal_save))
    elif universal_fit is not None or universal_load is not None or universal_save is not None:
        raise ValueError("universal_fit / universal_load / universal_save need a universal attack (AttackEnum UAP*)")
    if isinstance(atk, MultiAttack):
        reports.append(_MultiAttackReport(atk))
    if channel is not None:
        reports.append(_ChannelScorer(channel, channel_draws, device, seed))
    if certify is not None:
        reports.append(_CertifyScorer(certify, certify_samples, certify_select, certify_alpha, device, seed, rank_and_world()[0],
                                      attacked=atk is not None))
    return reports


def adopt_certify_sigma(atk, certify: Optional[float]) -> bool:
    """There is one smoothed detector per run: with `certify=sigma`, an attack on the smoothed detector
    (torchattacks.SmoothAdvPGD) attacks the one being certified, whatever sigma it was constructed with.  True when it applied."""
    from .torchattacks import SmoothAdvPGD
    if certify is None or not isinstance(atk, SmoothAdvPGD):
        return False
    LOGGER.info(f"SmoothAdvPGD: sigma {atk.sigma:g} -> {float(certify):g}, the smoothed detector this run certifies")
    atk.sigma = float(certify)
    return True


def _log_report(report: Dict[str, float], reports: List[_Report]) -> None:
    for line in ([r.line(report) for r in reports if r.leads] + [format_report(report)]
                 + [r.line(report) for r in reports if not r.leads]):
        LOGGER.info(line)

# ---------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------

def _device_batches(loader, device):
    """The loader's batches with `batch_x` / `batch_y` already on the device, ONE BATCH AHEAD of the consumer.

    A pageable host->device copy on the compute stream waits for everything queued there — the previous batch's whole
    attack — and blocks the host meanwhile, so neither the copy nor the collation of the next batch overlaps the GPU.
    Here the next batch is staged through one of two persistent pinned buffers and copied on a side stream (ragged
    `device_pad` batches: uploaded and decoded + padded there) while the current batch's kernels run; the compute stream
    only waits for that stream's event.  CPU devices pass through unchanged."""
    dev = torch.device(device)
    if dev.type != "cuda":
        for batch_x, batch_sr, batch_y, meta in loader:
            yield batch_x.to(dev), batch_sr, batch_y.to(dev), meta, None
        return
    side = torch.cuda.Stream(dev)
    pinned, done, slot = {}, [None, None], 0

    def stage(batch):
        nonlocal slot
        batch_x, batch_sr, batch_y, meta = batch
        with torch.cuda.stream(side):
            if isinstance(batch_x, RaggedWaveBatch):
                # device_pad datasets: the file payloads go up as they are; decode + first channel + pad/tile on the device
                x_dev = batch_x.to_padded(dev, WAVE_FAKE_CUT)
            else:
                key = (tuple(batch_x.shape), batch_x.dtype)
                if key not in pinned:
                    pinned[key] = [torch.empty(batch_x.shape, dtype=batch_x.dtype, pin_memory=True) for _ in range(2)]
                if done[slot] is not None:
                    done[slot].synchronize()          # the previous upload from this staging buffer has finished
                buf = pinned[key][slot]
                buf.copy_(batch_x)
                x_dev = buf.to(dev, non_blocking=True)
            y_dev = batch_y.to(dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        done[slot] = ev
        slot ^= 1
        return x_dev, batch_sr, y_dev, meta, ev

    it = iter(loader)
    try:
        ahead = stage(next(it))
    except StopIteration:
        return
    while ahead is not None:
        x_dev, batch_sr, y_dev, meta, ev = ahead
        # the consumer's stream for this batch waits for the upload (`_Lanes.batch`): with two batches in flight that is not
        # the stream this generator happens to run under
        yield x_dev, batch_sr, y_dev, meta, ev
        # resumed when the consumer asks for the next batch, i.e. after it has queued this batch's kernels: the
        # collation + upload below run behind them
        try:
            ahead = stage(next(it))
        except StopIteration:
            ahead = None


class _Lanes:
    """Batches in flight (round 6).  Batches of the evaluation loop are independent (reference
    :211-265: per-row min-max, per-batch dB floor, per-row attack state), and one PGD iteration leaves most of the 256 CUs
    idle for ~ 10 % of its time (the recurrent layers: 256 workgroups of 25 dependent steps; launch-sized GEMMs; the last,
    small convolution blocks).  With `n` = 2 batch i runs on stream i % 2, each stream replaying its own captured graph
    (torchattacks/graphed.py keys captures by launch stream), and the hardware fills one batch's idle CUs with the other's
    convolutions: configs[1] 69.1 -> 63.0 ms per batch (+ 9.6 %), scores bit-identical (tools/two_stream_probe.py).

    Ordering rules.  (1) A batch waits for its own upload event.  (2) Caches derived from the weights or from a batch shape
    (prepared Winograd weights, fragment tables, captured graphs) are built by whichever stream meets them first and are
    NOT ordered against other streams; so a batch runs behind everything queued before it — it waits for the previous
    batch's end event — until its (stream, batch shape) has been seen twice, i.e. until after that stream's capture.  From
    then on the two streams only read those caches.  (3) `join()` puts the caller's stream behind every lane before the
    scores are concatenated.  n = 1: the caller's stream, no extra synchronisation (rounds 1-5 behaviour)."""

    def __init__(self, device, n: int):
        self.dev = torch.device(device)
        self.cuda = self.dev.type == "cuda"
        self.n = max(1, int(n)) if self.cuda else 1
        self.main = torch.cuda.current_stream(self.dev) if self.cuda else None
        self.streams = [torch.cuda.Stream(self.dev) for _ in range(self.n)] if self.n > 1 else [self.main]
        self.seen: Dict[tuple, int] = {}
        self.prev_end = None
        self.held = []                                  # tensors produced on a lane and read by the caller's stream after join()
        if self.n > 1:
            for s in self.streams:
                s.wait_stream(self.main)

    def lane_of(self, i: int) -> int:
        return i % self.n

    @contextlib.contextmanager
    def batch(self, i: int, shape_key, ready=None, inputs=()):
        if not self.cuda:
            yield 0
            return
        k = self.lane_of(i)
        stream = self.streams[k]
        if ready is not None:
            stream.wait_event(ready)
        for t in inputs:
            t.record_stream(stream)
        if self.n == 1:
            yield 0
            return
        key = (k, shape_key)
        warm = self.seen.get(key, 0) >= 2
        self.seen[key] = self.seen.get(key, 0) + 1
        if not warm and self.prev_end is not None:
            stream.wait_event(self.prev_end)            # rule (2): behind everything queued so far
        with torch.cuda.stream(stream):
            yield k
            end = torch.cuda.Event()
            end.record(stream)
        self.prev_end = end

    def keep(self, *tensors):
        if self.n > 1:
            self.held.extend(tensors)

    def join(self):
        if self.n > 1:
            for s in self.streams:
                self.main.wait_stream(s)
            for t in self.held:
                t.record_stream(self.main)
            self.held = []


def prepare_universal(atk, loader, device, n_batches: int, fit: Optional[int] = None, load=None, save=None) -> int:
    """Give a universal attack (`is_universal`) its perturbation before the loop, on the caller's stream: from the file `load`,
    or by `atk.fit` on the first `fit` batches of `loader` (None: max(1, n_batches // 4)), normalised as the loop normalises
    them and KEPT ON THE DEVICE with their labels, mn and mx for the attack's epochs — fit x B x T x 4 bytes (66 MB for two
    batches of 128 utterances of 64 600 samples).  `save`: rank 0 writes the perturbation the run uses.  Returns the number of
    this rank's utterances it was fitted on (0 for a loaded one).  Fitting is single-process: every rank of a larger job loads
    the same file, so no step of the fit communicates."""
    rank, world = rank_and_world()
    fitted_rows = 0
    if load is not None:
        atk.load_delta(load)
    else:
        if world > 1:
            raise ValueError("a universal perturbation is fitted by one process: with more than one rank, fit it in a "
                             "single-process run with universal_save and pass that file as universal_load")
        n_fit = max(1, n_batches // 4) if fit is None else int(fit)
        if not 1 <= n_fit <= n_batches:
            raise ValueError(f"universal_fit must name between 1 and the run's {n_batches} batches, got {n_fit}")
        dev = torch.device(device)
        kept = []
        batches = _device_batches(loader, device)
        for batch_x, _, batch_y, _, ready in batches:
            if ready is not None:                          # uploaded on a side stream: this stream waits and takes the tensors over
                torch.cuda.current_stream(dev).wait_event(ready)
                batch_x.record_stream(torch.cuda.current_stream(dev))
                batch_y.record_stream(torch.cuda.current_stream(dev))
            x01, mn, mx = aa_utils.to_minmax(batch_x)
            kept.append((x01, batch_y, mn, mx))
            fitted_rows += batch_x.size(0)
            if len(kept) == n_fit:
                break
        batches.close()
        atk.reset()
        atk.fit(kept)
    if save is not None and rank == 0:
        atk.save_delta(save)
    return fitted_rows


def default_in_flight(atk, device, has_callback: bool) -> int:
    """Two batches in flight when the attack's inner loop replays from a hipGraph (PGD, PGDL2: the host queues a batch in a
    few milliseconds); host-driven attacks (CW: a host read every steps // 10 iterations; FAB) and callback runs (the
    analyser reads every batch back) stay at one.  ADVSTEP_IN_FLIGHT overrides."""
    env = os.environ.get("ADVSTEP_IN_FLIGHT")
    if env:
        return max(1, int(env))
    if atk is None or has_callback or torch.device(device).type != "cuda":
        return 1
    from .torchattacks import graphed
    return 2 if (getattr(atk, "replays_from_graph", False) and graphed.enabled()) else 1


def get_dataset(datasets_paths: List[Union[str, os.PathLike, None]], amount_to_use: Optional[int],
                raw_sample_from_dataset: bool = False, device_pad: bool = False,
                wave_fake_trim: Optional[bool] = None) -> DetectionDataset:
    """Reference :301-317 — the validation part of the three corpora, class-balanced, optionally reduced."""
    return DetectionDataset(asvspoof_path=datasets_paths[0], wavefake_path=datasets_paths[1],
                            fakeavceleb_path=datasets_paths[2], subset="val", reduced_number=amount_to_use,
                            return_label=True, return_meta=True, return_raw=raw_sample_from_dataset,
                            device_pad=device_pad, wave_fake_trim=wave_fake_trim)


def generate_attacks(
    datasets_paths: List[Union[str, os.PathLike, None]],
    model_config: Dict,
    device: str,
    attack_model_config: Optional[Dict] = None,
    attack_method: Optional[Any] = None,
    attack_params: Dict = {},
    amount_to_use: Optional[int] = None,
    batch_size: int = 64,
    on_attack_end_callback: Optional[Callable] = None,
    raw_sample_from_dataset: bool = False,
    dataset: Optional[Dataset] = None,
    share_weights: bool = False,
    shuffle: bool = True,
    num_workers: int = 3,
    device_pad: bool = True,
    wave_fake_trim: Optional[bool] = None,
    return_scores: bool = False,
    on_batch_queued: Optional[Callable[[int], None]] = None,
    in_flight: Optional[int] = None,
    perturbation_stats: bool = False,
    universal_fit: Optional[int] = None,
    universal_load: Optional[Union[str, os.PathLike]] = None,
    universal_save: Optional[Union[str, os.PathLike]] = None,
    channel: Optional[Any] = None,
    channel_draws: int = 1,
    masking_stats: bool = False,
    certify: Optional[float] = None,
    certify_samples: int = 1000,
    certify_select: int = 100,
    certify_alpha: float = 0.001,
) -> Dict[str, float]:
    """Reference signature (:146-157) plus additive keywords: `dataset` (a ready Dataset yielding the reference's
    4-tuple; without it the `DetectionDataset` over `datasets_paths` is built as in the reference's `get_dataset`,
    :301-317, or — with no corpus path — `amount_to_use` synthetic utterances are generated), `share_weights`
    (white-box runs without checkpoints: copy the target's weights into the attack model), `shuffle`, `num_workers` (3 like the reference, :202 — the loop is launch-bound on the host,
    so collation belongs in worker processes),
    `device_pad` (real corpora: ship undecoded payloads and pad on the device) and `wave_fake_trim` (None = the
    reference's default, the SoX silence trim, which needs a registered backend) and `return_scores` (adds the whole job's
    per-utterance `y_pred`, `y_pred_label`, `y` arrays, in rank order, and every optional report's own rows to the returned
    report under "scores") and
    `on_batch_queued(i)` (called when batch i's kernels have been queued, under the stream they were queued on — no
    synchronisation, no extra work: measurements) and `in_flight` (batches processed concurrently on streams of their own,
    `_Lanes`; None = `default_in_flight`: 2 for the graph-replayed attacks, else 1; same scores either way).
    The remaining keywords, and some attacks by what they carry, add optional reports: keys behind the reference's, one more log
    line each and rows under "scores" (`_active_reports` lists them; without any, the report, the launches of a batch and the
    log are those of the reference's loop).  `perturbation_stats`: the per-utterance L-inf, L2, SNR and segmental SNR of what
    the attack did.  `universal_fit` / `universal_load` / `universal_save`: where a universal attack's perturbation comes from
    and goes (`_UniversalReport`); any other attack: they must be left at None.  `channel`, `channel_draws`: what is left of the
    attack after that many draws of a simulated audio channel (`_ChannelScorer`).  `masking_stats`: every attack's perturbation
    rated against the clean utterance's psychoacoustic masking threshold (`masking_pass`).  `certify` (a noise level sigma > 0, in
    the waveform's units), `certify_samples` (n), `certify_select` (n0), `certify_alpha`: randomized smoothing's certified L2
    radius of every clean utterance and, with an attack, the smoothed detector's answer to it (`_CertifyScorer`).
    `batch_size` is the GLOBAL batch."""
    rank, world = rank_and_world()
    LOGGER.info("Loading data...")

    model = load_model(model_config, device)                       # :162  (no DataParallel: one process per GPU)
    if attack_model_config is not None and attack_method is not None:
        attack_model = load_model(attack_model_config, device)     # :166
        if share_weights:
            attack_model.load_state_dict(model.state_dict())
        atk = attack_method(attack_model, **attack_params)         # :169
        atk.set_training_mode(model_training=True, batchnorm_training=False)  # :170
        adopt_certify_sigma(atk, certify)
    else:
        attack_model, atk = None, None

    if dataset is None:
        if any(p is not None for p in datasets_paths):
            dataset = get_dataset(datasets_paths, amount_to_use, raw_sample_from_dataset, device_pad=device_pad,
                                  wave_fake_trim=wave_fake_trim)
        else:
            dataset = SyntheticDetectionDataset(amount_to_use if amount_to_use else 4 * batch_size)
    data_val = dataset
    collate_fn = ragged_collate if getattr(data_val, "device_pad", False) else None

    LOGGER.info(f"Testing '{model.__class__.__name__}' model, weights path: '{model.weights_path}', "
                f"on {len(data_val)} audio files.")
    if attack_model is not None:
        LOGGER.info(f"Attack using '{attack_model.__class__.__name__}' model and '{atk.__class__.__name__}' method "
                    f"({attack_params}), weights path: '{attack_model.weights_path}'")
    else:
        LOGGER.info("No attack applied")

    seed = model_config.get("data", {}).get("seed", 42)
    sampler = ShardedBatchSampler(len(data_val), batch_size, rank, world, shuffle=shuffle, seed=seed)
    # (pinning every (B, 64600) float batch was measured and costs more than it saves — a fresh pinned allocation per batch
    # on the launching thread: 1 082 -> 737 utt/s without workers; only the small ragged payloads are pinned)
    test_loader = DataLoader(data_val, batch_sampler=sampler, num_workers=num_workers, collate_fn=collate_fn,
                             pin_memory=collate_fn is not None)
    if world > 1:
        # decorrelate the random starts of different ranks (all ranks were seeded alike to build equal replicas)
        torch.manual_seed(seed + rank)

    # BEFORE the lanes exist: a universal fit runs on the caller's stream, and the lanes' constructor orders every lane behind it
    reports = _active_reports(atk, device, seed + rank, test_loader, len(sampler), perturbation_stats, masking_stats, channel,
                              channel_draws, universal_fit, universal_load, universal_save, certify, certify_samples,
                              certify_select, certify_alpha)
    lanes = _Lanes(device, in_flight if in_flight is not None
                   else default_in_flight(atk, device, on_attack_end_callback is not None))
    num_correct = [torch.zeros((), dtype=torch.int64, device=device) for _ in range(lanes.n)]
    seen_total = 0
    y_pred, y_pred_label, y = [], [], []

    def preprocessed(x):  # :229-234 — the dataset's default preprocessing, at the CURRENT batch's sampling rates
        return SimpleAudioFakeDataset.wavefake_preprocessing_on_batch(x, batch_sr, wave_fake_trim=wave_fake_trim)[0]
    post = preprocessed if raw_sample_from_dataset else None

    for i, (batch_x, batch_sr, batch_y, batch_metadata, ready) in enumerate(_device_batches(test_loader, device)):
      with lanes.batch(i, tuple(batch_x.shape), ready, (batch_x, batch_y)) as lane:
        model.eval()
        seen_total += batch_x.size(0)

        if attack_model is not None:
            batch_x_attacked = attack_batch(atk, batch_x, batch_y)
        else:
            batch_x_attacked = torch.clone(batch_x)
        batch_x_noproc, batch_x_attacked_noproc = batch_x, batch_x_attacked  # :223-224 (nothing below writes in place)
        for r in reports:
            lanes.keep(*r.batch(atk, batch_x, batch_x_attacked))

        if raw_sample_from_dataset:  # after the attack
            batch_x_attacked = preprocessed(batch_x_attacked)
        batch_preds, batch_preds_label = score_batch(model, batch_x_attacked)
        for r in reports:
            lanes.keep(*r.scored(lane, model, batch_x_noproc, batch_x_attacked_noproc, batch_y, batch_preds_label, post))

        if on_attack_end_callback is not None:  # :240-259
            if raw_sample_from_dataset:
                batch_x = preprocessed(batch_x)
            batch_preds_noattack, batch_preds_noattack_label = score_batch(model, batch_x)
            on_attack_end_callback(batch_x=batch_x_noproc, batch_x_attacked=batch_x_attacked_noproc, batch_y=batch_y,
                                   batch_preds_label=batch_preds_label, batch_preds=batch_preds,
                                   batch_preds_noattack_label=batch_preds_noattack_label,
                                   batch_preds_noattack=batch_preds_noattack, batch_metadata=batch_metadata)

        num_correct[lane] += (batch_preds_label == batch_y.int()).sum()
        y_pred.append(batch_preds)
        y_pred_label.append(batch_preds_label)
        y.append(batch_y)
        lanes.keep(batch_preds, batch_preds_label, batch_y)
        if on_batch_queued is not None:
            on_batch_queued(len(y) - 1)

    lanes.keep(*num_correct)
    lanes.join()
    num_correct = num_correct[0] if lanes.n == 1 else torch.stack(num_correct).sum()
    num_total = torch.tensor(seen_total, dtype=torch.int64, device=device)
    if not y:
        raise ValueError(f"no complete batch: {len(data_val)} items < global batch {batch_size} (drop_last=True)")
    all_pred, all_label, all_y, n_correct, n_total = aggregate_across_ranks(
        torch.cat(y_pred), torch.cat(y_pred_label), torch.cat(y), num_correct, num_total)

    report = metrics.adversarial_report(all_y, all_pred, all_label)
    report["adv_eval/accuracy"] = (n_correct / n_total) * 100  # :267 (from the all-reduced counters)
    report["num_total"] = n_total
    if return_scores:
        report["scores"] = {"y_pred": all_pred, "y_pred_label": all_label, "y": all_y}
    ctx = SimpleNamespace(all_y=all_y, all_label=all_label, samples=batch_x_noproc[0].numel(), rank=rank, world=world, device=device)
    for r in reports:
        report.update(r.finish(ctx))
        if return_scores:
            report["scores"].update(r.scores())
    if rank == 0:
        _log_report(report, reports)
    return report
