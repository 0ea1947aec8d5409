"""HopSkipJump: the label-only black-box attack (no counterpart in the reference, whose every attack differentiates the attacked
detector)."""
import math

import numpy as np
import torch

from ..attack import Attack


class HopSkipJump(Attack):
    r"""HopSkipJump (Chen, Jordan and Wainwright, IEEE S&P 2020) in its L-inf form.  The attacker submits waveforms and reads only
    the detector's DECISION, "bona fide" or "spoof"; the figures the attack adds beside the robust accuracy are each utterance's
    RADIUS (how close to it a label-only attacker gets) and its QUERIES.

    A logit z is adversarial for row b iff (z > 0) != (y[b] == 1) (SPSA's rule: +-0 and NaN are class 0).  `cur` is the row's
    current adversarial point, dist = max |cur - x| (plane 0 of `ops.perturbation_stats`), and
    point(r) = clamp(x + clamp(cur - x, -r, r), 0, 1).

        0. Start: x is scored (1 query).  A row already misclassified is finished: x, radius 0.  Every other row takes a DONOR as
           cur, the first other row of the batch, in cyclic order from b + 1, that the detector assigns to the other class (an
           attacker owns recordings of both classes).  Rows without a donor try `init_trials` uniform-noise rows (uniform on the
           2^-16 grid of [0, 1], drawn on the device from a generator seeded with the call's seed; one query each for those
           rows), the first adversarial one wins.  A row with no start returns x with radius +inf.
        1. Boundary search, after the start and after every step: `search_steps` rounds of bisection on r in [0, dist]
           (`ops.hsj_search_open` / `_next` / `_close`, one launch per query, the state is device data); where a probe was
           adversarial cur becomes point(hi), the bytes of that probe, otherwise cur keeps its bytes.
        2. Normal estimate at iteration t = 1 .. steps: n_t = min(max_evals, int(init_evals sqrt(t))) probes
           clamp(cur +- m, 0, 1) with Rademacher signs (`ops.hsj_probe`, SPSA's Philox directions, never stored), in chunks of at
           most `max_rows` forward rows; m = max(delta_rel * dist, delta_min) per row.
        3. Step: `ops.hsj_candidates` forms the sign s of the estimate from the n_t DECISIONS and writes `step_trials` candidates
           clamp(cur + (xi 2^-k) s, 0, 1), xi = dist * xi_rel_t, xi_rel_t = float32(1 / sqrt(t)) or `step_schedule[t - 1]`; they
           are scored together and `ops.hsj_take` takes the first adversarial one (the largest step), counting the k + 1 queries
           a sequential attacker would have spent; if none is adversarial the row stays and step_trials queries are counted.
        4. dist is recomputed, the boundary search runs, then the next iteration.

    Departures from the paper, all forced by float32 on 64 600-sample rows or by fixed shapes:
        * L-inf only, Rademacher instead of Gaussian directions, so the probes are cur +- m exactly, one rounding per sample;
        * the probe size is relative to dist with a floor (`delta_rel`, `delta_min`), not the paper's dist / d over a unit-L2
          vector, which is below one ulp of a sample here;
        * the estimate sum_j (phi_j - mean phi) v_j is evaluated as the integer c e - (n - c) a (include/advstep_hsj.h): exact,
          order-free, and two population counts per 8 directions;
        * a fixed number of bisection rounds instead of a threshold, and a fixed set of `step_trials` halvings scored in one
          forward instead of the paper's open-ended halving loop;
        * the start is a donor from the batch before it is noise, and the donor is not blended towards x by a separate search
          (the first boundary search does that).

    A row is ACTIVE while it has a start and, with `early_stop`, dist > eps.  Inactive rows are still forwarded (the batch shape
    never changes); every kernel writes cur's bytes for them and counts no query.  There is no host read inside `forward`.

    Arguments:
        model (nn.Module): model to attack.
        eps (float or None): the radius a row must reach; rows that reach it are returned, the others come back as x.
            None: every row with a start is returned at whatever radius it reached, and nothing stops early. (Default: 0.0005)
        steps (int): iterations. (Default: 10)
        init_evals (int), max_evals (int): n_t = min(max_evals, int(init_evals sqrt(t))), at most
            `hip_ops.HSJ_MAX_DIRECTIONS`. (Default: 32, 256)
        search_steps (int): bisection rounds of one boundary search. (Default: 12)
        step_trials (int): candidate steps per iteration, at most `hip_ops.HSJ_MAX_TRIALS`. (Default: 4)
        delta_rel (float), delta_min (float): probe size max(delta_rel * dist, delta_min). (Default: 2^-6, 2^-16)
        init_trials (int): noise starts tried for rows without a donor. (Default: 8)
        step_schedule (sequence of float or None): xi_rel per iteration, at least `steps` long. (Default: None)
        max_rows (int): forward rows per model call. (Default: 1024)
        early_stop (bool): freeze rows whose dist is within eps. (Default: True)
        report_at (tuple): radii at which `evaluation.generate_attacks` reports the robust accuracy. (Default: ())

    After a call `last_radius` holds (B,) float32 on the device — 0 for a row that was wrong from the start, dist for a row with a
    start, +inf otherwise — and `last_queries` (B,) int32.  `budget` = 1 + (steps + 1) search_steps + sum_t (n_t + step_trials) is
    what a row that starts from a donor and never stops spends at most (a step that succeeds at slot k counts k + 1 of its
    step_trials); noise trials come on top.

    Only the default (untargeted) mode is supported.  The loop is eager: graph capture and two batches in flight are out of scope.

    Examples::
        >>> attack = torchattacks.HopSkipJump(model, eps=0.0005, steps=10)
        >>> adv_images = attack(images, labels)
        >>> radii, queries = attack.last_radius, attack.last_queries
    """

    replays_from_graph = False

    def __init__(self, model, eps=0.0005, steps=10, init_evals=32, max_evals=256, search_steps=12, step_trials=4,
                 delta_rel=2.0 ** -6, delta_min=2.0 ** -16, init_trials=8, step_schedule=None, max_rows=1024, early_stop=True,
                 report_at=()):
        super().__init__("HopSkipJump", model)
        if eps is not None and not float(eps) >= 0.0:                # (a NaN eps fails the comparison)
            raise ValueError(f"eps must be a radius >= 0 or None, got {eps}")
        if min(int(steps), int(init_evals), int(max_evals), int(search_steps), int(step_trials), int(max_rows)) < 1:
            raise ValueError("steps, init_evals, max_evals, search_steps, step_trials and max_rows must be at least 1, got "
                             f"{steps}, {init_evals}, {max_evals}, {search_steps}, {step_trials} and {max_rows}")
        if int(max_evals) > 1024 or int(step_trials) > 8:           # hip_ops.HSJ_MAX_DIRECTIONS, HSJ_MAX_TRIALS
            raise ValueError(f"max_evals is at most 1024 and step_trials at most 8, got {max_evals} and {step_trials}")
        if int(init_trials) < 0:
            raise ValueError(f"init_trials must be >= 0, got {init_trials}")
        if not (float(delta_rel) >= 0.0 and float(delta_min) >= 0.0 and max(float(delta_rel), float(delta_min)) > 0.0):
            raise ValueError(f"delta_rel and delta_min must be >= 0 and not both 0, got {delta_rel} and {delta_min}")
        if step_schedule is not None:
            step_schedule = tuple(float(v) for v in step_schedule)
            if len(step_schedule) < int(steps) or not all(v > 0.0 for v in step_schedule):
                raise ValueError(f"step_schedule needs {steps} positive entries, got {step_schedule}")
        self.eps = eps
        self.steps = steps
        self.init_evals = init_evals
        self.max_evals = max_evals
        self.search_steps = search_steps
        self.step_trials = step_trials
        self.delta_rel = delta_rel
        self.delta_min = delta_min
        self.init_trials = init_trials
        self.step_schedule = step_schedule
        self.max_rows = max_rows
        self.early_stop = early_stop
        self.report_at = tuple(report_at)
        self._supported_mode = ["default"]
        self._last_radius = None
        self._last_queries = None

    def evals(self, t):
        """n_t: the probes of iteration t = 1 .. steps."""
        return min(int(self.max_evals), int(int(self.init_evals) * math.sqrt(t)))

    def step_size(self, t):
        """xi_rel_t as the float32 the kernel receives."""
        v = 1.0 / math.sqrt(t) if self.step_schedule is None else self.step_schedule[t - 1]
        return float(np.float32(v))

    @property
    def budget(self):
        """1 + (steps + 1) search_steps + sum_t (n_t + step_trials): the queries of a row that starts from a donor and is never
        frozen, every step counted in full.  Noise trials are not in the budget."""
        steps = int(self.steps)
        return 1 + (steps + 1) * int(self.search_steps) + sum(self.evals(t) + int(self.step_trials) for t in range(1, steps + 1))

    @property
    def last_radius(self):
        """The radii of the last call, (B,) float32 on the device (None before the first call); not a hyper-parameter."""
        return self._last_radius

    @property
    def last_queries(self):
        """The queries of the last call, (B,) int32 on the device (None before the first call); not a hyper-parameter."""
        return self._last_queries

    def _score(self, rows, out=None):
        """The logits of `rows` (N, ...), (N,), in pieces of at most max_rows; into `out` when given."""
        N, max_rows = rows.shape[0], int(self.max_rows)
        if out is None:
            out = torch.empty(N, dtype=torch.float32, device=rows.device)
        with torch.no_grad():
            for r0 in range(0, N, max_rows):
                z = self.model(rows[r0:r0 + max_rows])
                if z.dim() != 2 or z.shape[1] != 1:
                    raise ValueError(f"the attacked model must emit one logit per utterance, got {tuple(z.shape)}")
                out[r0:r0 + max_rows] = z.reshape(-1)
        return out

    def forward(self, images, labels):
        r"""
        Overridden.
        """
        ops = self.ops
        images, labels, _ = self._prepare(images, labels)
        y = labels.to(torch.int64).reshape(-1).contiguous()
        shape, device = tuple(images.shape), images.device
        B = shape[0]
        T = images.numel() // B if B else 0
        steps, R, K = int(self.steps), int(self.search_steps), int(self.step_trials)
        max_rows = int(self.max_rows)
        seed = self._fresh_seed()
        x = images.reshape(B, T)
        is_one = y == 1

        def full(rows):                                              # (N, T) -> the model's input shape
            return rows.reshape((rows.shape[0],) + shape[1:])

        def stats():
            """(dist, active): plane 0 of the perturbation report, and the rows that still move."""
            dist = ops.perturbation_stats(x, cur)[0].contiguous()
            moving = has_start if (self.eps is None or not self.early_stop) else has_start & ~(dist <= float(self.eps))
            return dist, moving.to(torch.int32)

        # ---- 0. start -------------------------------------------------------------------------------------------------------
        z0 = self._score(images)
        queries = torch.ones(B, dtype=torch.int32, device=device)
        other = z0 > 0                                               # the detector's class of every row
        wrong = other != is_one                                      # finished: x at radius 0
        # row b's candidates in cyclic order from b + 1; the first whose class is not y[b]
        order = (torch.arange(B, device=device)[:, None] + 1 + torch.arange(max(B - 1, 1), device=device)[None, :]) % max(B, 1)
        fits = (other[order] != is_one[:, None]) & (B > 1)
        has_donor = fits.any(dim=1) & ~wrong
        donor = torch.gather(order, 1, fits.to(torch.int8).argmax(dim=1, keepdim=True)).reshape(-1)
        cur = torch.where(has_donor[:, None], x[donor], x).contiguous()
        has_start = has_donor.clone()
        if int(self.init_trials) > 0:
            gen = torch.Generator(device=device)
            gen.manual_seed(seed)
            for _ in range(int(self.init_trials)):
                need = ~wrong & ~has_start
                # uniform on the 2^-16 grid of [0, 1]: what a 16-bit recording of noise holds
                noise = torch.randint(0, 2 ** 16 + 1, (B, T), generator=gen, device=device).to(torch.float32) * 2.0 ** -16
                take = need & ((self._score(full(noise)) > 0) != is_one)
                cur = torch.where(take[:, None], noise, cur)
                has_start = has_start | take
                queries += need.to(torch.int32)
        cur = cur.contiguous()

        # ---- buffers ----------------------------------------------------------------------------------------------------------
        n_max = max(self.evals(t) for t in range(1, steps + 1))
        per_chunk = max(1, min(n_max, max_rows // max(B, 1)))       # probe slots per fill
        probe = torch.empty_like(cur)
        states = torch.empty((2, 4, B), dtype=torch.float32, device=device)
        probes = torch.empty((per_chunk, B, T), dtype=torch.float32, device=device)
        cand = torch.empty((K, B, T), dtype=torch.float32, device=device)
        z = torch.empty((n_max, B), dtype=torch.float32, device=device)
        zc = torch.empty((K, B), dtype=torch.float32, device=device)

        def search(dist, active):
            """§1: R queries per active row; cur is updated in place."""
            which = 0
            ops.hsj_search_open(cur, x, dist, active, probe, state=states[0])
            for rnd in range(R):
                zr = self._score(full(probe))
                if rnd < R - 1:
                    ops.hsj_search_next(cur, x, zr, y, active, states[which], probe, state_out=states[1 - which])
                    which = 1 - which
                else:
                    ops.hsj_search_close(cur, x, zr, y, active, states[which], queries, R, out=cur)

        dist, active = stats()
        search(dist, active)
        dist, active = stats()

        # ---- the iterations ---------------------------------------------------------------------------------------------------
        offset = 0
        for t in range(1, steps + 1):
            n = self.evals(t)
            mag = torch.clamp(dist * float(self.delta_rel), min=float(self.delta_min)).contiguous()
            zt = z[:n]
            zt_flat = zt.reshape(-1)
            for s0 in range(0, n, per_chunk):
                ns = min(per_chunk, n - s0)
                chunk = probes[:ns]
                ops.hsj_probe(cur, mag, active, seed, offset, s0=s0, ns=ns, out=chunk)
                self._score(full(chunk.reshape(ns * B, T)), out=zt_flat[s0 * B:(s0 + ns) * B])
            ops.hsj_candidates(cur, zt, y, dist, active, self.step_size(t), K, seed, offset, out=cand)
            self._score(full(cand.reshape(K * B, T)), out=zc.reshape(-1))
            ops.hsj_take(cur, cand, zc, y, active, queries, n, out=cur)
            offset += (n + 31) // 32
            dist, active = stats()
            search(dist, active)
            dist, active = stats()

        inf = torch.full_like(dist, math.inf)
        self._last_radius = torch.where(wrong, torch.zeros_like(dist), torch.where(has_start, dist, inf))
        self._last_queries = queries
        keep = has_start if self.eps is None else has_start & (dist <= float(self.eps))
        return torch.where(keep[:, None], cur, x).reshape(shape)
