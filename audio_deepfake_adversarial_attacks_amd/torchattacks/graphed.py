"""hipGraph replay of the iterative attacks' inner loop (PGD, PGDL2, MIFGSM, NIFGSM).

One attack iteration on LCNN is ~37 kernel launches (model forward + input-backward through the fused kernels, the
closed-form loss gradient, the fused update step) of fixed shapes; launched eagerly the launching thread is busy for as
long as the GPU is, so with the data loader's collation on the same thread — or eight ranks sharing one host — the loop
turns host-bound.  Here the MODEL PART of an iteration — forward, loss gradient, input-backward —
is captured once per (model state, batch shape, attack hyper-parameters, launch stream) into two hipGraphs, one reading
each of the two ping-pong buffers, and the update step is launched between the replays:
    replay G_a: grad_a = d cost / d adv_a      step(adv_a, grad_a) -> adv_b
    replay G_b: grad_b = d cost / d adv_b      step(adv_b, grad_b) -> adv_a            (steps / 2 times)
Round 6: rounds 2-5 captured BOTH iterations including their steps in one graph ("fused", still behind
ADVSTEP_ATTACK_GRAPH=fused for A/B).  The split form costs the host one more graph launch and two plain launches per pair
(microseconds against a 3.4 ms pair) and buys two things: the step kernel — the kernel bench.py prices — can be bracketed
with HIP events while the loop replays (events cannot be recorded into a graph), so the measured loop IS the shipped loop;
and nothing of the launch stream's scratch is baked into a graph.

Two batches in flight (round 6, evaluation.generate_attacks / bench.py): the key carries the LAUNCH STREAM, so two streams
that alternate batches get a capture each — a capture owns its static buffers and its activation pool and cannot serve
two batches at once — over the same read-only model.

What is baked into a captured graph and therefore part of its key: the device pointers of the static input buffers (owned
here), of the model's parameters and buffers and of every cache derived from them (prepared Winograd weights, `bn_eval_affine`
pairs, RawNet3's chain plans, packed GRU weights, filterbank tables).  The key has two parts:
    family  what makes two calls the same workload AND may come back: the model's identity, the attack class and its
            hyper-parameters, targeted mode, the batch shape, the labels' dtype / shape, the launch stream, the graph form, every
            module's train/eval flag and every ADVSTEP_* switch (an A/B run flips a switch and flips it back; an attack in eval
            mode alternates with one in train mode on the same model);
    state   the (address, version counter) of every parameter and buffer.  Version counters only grow: a capture under an
            older state can never be replayed again.
A graph is captured only when the same key shows up a second time (an adversarial-training step changes the weights before
every attack call: those calls stay eager), and capturing a family under a new state drops the captures of the same family
under older states (each holds a private memory pool).  Captures of one workload under other flags or switches are kept,
so the caches they bake must stay where they are while the other path runs: the caches are keyed by parameter / buffer
versions, not by the switches, and the one that is built per switch value, a residual block's plan under
ADVSTEP_RESBLOCK_FEW, keeps a plan per value (detector_ops.res_block_plan).  Random starts are drawn OUTSIDE the graph (a
fresh Philox key per call).

Lifetime: a capture dies with its model.  The tables are keyed by id(model), an integer that CPython hands to the next object
at that address, and by addresses and version counters that an equally built later model can reproduce; a capture that
outlived its model would keep its private pool (the whole forward + backward activation set) and could be replayed for a
stranger.  So the first call on a model registers a `weakref.finalize` on it that drops the model's captures and its entries
in `_SEEN` / `_FAILED`.  No strong reference to the model is held here: that would keep the pool alive for good.

Hazards the suite pins (tests/test_gpu_graph_detectors.py on RawNet3, SpecRNet and LCNN; tests/test_graph_keys_host.py for the
pure parts): in-place parameter changes, buffer-only changes (BatchNorm running statistics), `load_state_dict` of equal values,
an ADVSTEP_* switch flipped and flipped back with live captures, train/eval flags, targeted mode, the labels' dtype, a partial
batch between replays, eviction at `_MAX_GRAPHS`, weights that change before every call, and the model's death.  Not run: a
failing capture (it would have to raise inside a stream capture); that branch is covered by reading.

Eager fallback, always bit-identical: CPU op tables / checked ops (tests), launch profiling of kernels INSIDE the model
part (hip_ops.start_profile without graph_ok: bench.py's per-family brackets), ADVSTEP_ATTACK_GRAPH=0, the attack's own off
switch (Attack._graph_off: MultiAttack's member calls on a sub-batch), or a failed capture."""
from __future__ import annotations

import os
import warnings
import weakref
from typing import Callable, Dict, Optional, Tuple

import torch

_GRAPHS: Dict[tuple, "_Captured"] = {}
_SEEN: Dict[tuple, int] = {}
_FAILED: set = set()          # family keys (model, attack, shape, hyper-parameters) whose capture failed: they stay eager
_MAX_GRAPHS = 8
_WATCHED: Dict[int, weakref.finalize] = {}     # id(model) -> the finalizer that drops the model's entries when it dies


def _toggles() -> Tuple:
    """Every ADVSTEP_* environment switch, sorted: the model's forward and the step kernels read them at call time, so a
    captured kernel sequence is only valid for the values it was captured under (A/B runs flip them between calls)."""
    return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("ADVSTEP_")))


def enabled() -> bool:
    return os.environ.get("ADVSTEP_ATTACK_GRAPH", "1") != "0"


def fused_form() -> bool:
    """ADVSTEP_ATTACK_GRAPH=fused: rounds 2-5's single graph of two whole iterations (A/B; cannot carry event brackets)."""
    return os.environ.get("ADVSTEP_ATTACK_GRAPH", "1") == "fused"


def _state_signature(model: torch.nn.Module) -> Tuple:
    versions = tuple((p.data_ptr(), p._version) for p in model.parameters())
    buffers = tuple((b.data_ptr(), b._version) for b in model.buffers())
    flags = tuple(m.training for m in model.modules())
    return versions, buffers, flags


def _forget_model(model_id: int) -> None:
    """Drop everything keyed by `model_id` (the first component of every family): captures with their pools, sightings, failures."""
    _WATCHED.pop(model_id, None)
    for table in (_GRAPHS, _SEEN):
        for key in [k for k in table if k[0] == model_id]:
            del table[key]
    for family in [f for f in _FAILED if f[0] == model_id]:
        _FAILED.discard(family)


def _watch(model: torch.nn.Module) -> None:
    """Tie the table entries of `model` to its lifetime (module docstring, "Lifetime").  The callback gets the id, not the
    model; not run at interpreter exit, where the HIP runtime may already be gone."""
    if id(model) not in _WATCHED:
        fin = weakref.finalize(model, _forget_model, id(model))
        fin.atexit = False
        _WATCHED[id(model)] = fin


class _Captured:
    def __init__(self, attack, images, labels, target, step_fn, fused: bool, step_has_state: bool = False):
        dev = images.device
        self.fused = fused
        self.images = torch.empty_like(images)
        self.adv_a = torch.empty_like(images)
        self.adv_b = torch.empty_like(images)
        self.labels = torch.empty_like(labels)
        self.target = torch.empty_like(target) if target is not None else None
        self.images.copy_(images), self.labels.copy_(labels), self.adv_a.copy_(images)
        if target is not None:
            self.target.copy_(target)
        # A step that owns per-call state (MI-FGSM's momentum) is never launched here, not even to warm up: only the iterations
        # of its own call may advance that state.  (Such steps stay out of the fused form: run_iterations.)
        warm_step = not step_has_state
        if not warm_step:
            self.adv_b.copy_(images)                         # the warm-up's second model pass reads it

        def two_iterations():
            grad, _ = attack._input_gradient(self.adv_a, self.labels, self.target)
            if warm_step:
                step_fn(self.adv_a.detach(), grad, self.images, self.adv_b)
            grad, _ = attack._input_gradient(self.adv_b, self.labels, self.target)
            if warm_step:
                step_fn(self.adv_b.detach(), grad, self.images, self.adv_a)

        # warm-up on a side stream (torch's capture protocol): builds every lazily created cache and workspace
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            two_iterations()
        torch.cuda.current_stream(dev).wait_stream(side)
        from .. import hip_ops
        # thread-local capture mode: with N > 1 ranks the RCCL watchdog thread (event queries), and in the CLI the DataLoader's
        # pinning thread, make HIP calls of their own while this thread captures; in the default "global" mode any such call
        # invalidates the capture
        # captured on the warm-up stream: everything keyed by the launch stream (hip_ops' row-reduction workspace) was created
        # by the warm-up, OUTSIDE the capture, so nothing that outlives this object is allocated from the graph's private pool
        if fused:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
                two_iterations()
        else:
            # the model part only; the gradients are the graphs' OUTPUTS: they live in the graphs' shared private pool and keep
            # their addresses as long as this object holds them.  G_b re-uses G_a's pool: the two never run at the same time
            # (one stream), so the second forward + backward's activations lie over the first's.
            self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_a, stream=side, capture_error_mode="thread_local"):
                self.grad_a, _ = attack._input_gradient(self.adv_a, self.labels, self.target)
            with torch.cuda.graph(self.graph_b, pool=self.graph_a.pool(), stream=side, capture_error_mode="thread_local"):
                self.grad_b, _ = attack._input_gradient(self.adv_b, self.labels, self.target)
        # A fused graph bakes in the ADDRESSES of hip_ops' row-reduction workspaces of (device, warm-up stream, batch shape): it
        # takes them OUT of hip_ops' table and owns them from here on — nothing hip_ops does later can free a buffer the graph
        # writes to on every replay, and no eager call on a stream that re-uses the warm-up stream's handle is ever given the same
        # buffer (one workspace, one stream: include/advstep.h).  (The split form's graphs contain no step kernel;
        # the warm-up's buffers simply leave the table with the stream.)
        self._workspaces = hip_ops.release_stream_workspaces(side.cuda_stream)

    def run(self, adv, images, labels, target, pairs: int, step_fn: Callable) -> torch.Tensor:
        # `step_fn` is the CURRENT call's: a closure may own per-call state, and the one of the capturing call is long done
        # (adv_a / adv_b became autograd leaves during the capture: write through detached views)
        self.images.copy_(images), self.labels.copy_(labels), self.adv_a.detach().copy_(adv)
        if target is not None:
            self.target.copy_(target)
        if self.fused:
            for _ in range(pairs):
                self.graph.replay()
            return self.adv_a.detach()
        a, b = self.adv_a.detach(), self.adv_b.detach()
        for _ in range(pairs):
            self.graph_a.replay()
            step_fn(a, self.grad_a, self.images, b)            # eager, on the launch stream: bracketable (hip_ops._Launch)
            self.graph_b.replay()
            step_fn(b, self.grad_b, self.images, a)
        return a


def run_iterations(attack, adv: torch.Tensor, images: torch.Tensor, labels: torch.Tensor, target: Optional[torch.Tensor],
                   steps: int, step_fn: Callable, hyper: Tuple, step_has_state: bool = False) -> torch.Tensor:
    """`steps` iterations of  adv <- step_fn(adv, grad(adv), images, out)  starting from `adv`; returns the final adv
    (detached, own storage).  step_fn(adv, grad, images, out) must write `out` (a different buffer than `adv`).
    step_has_state: the closure owns buffers of this call that it updates at every step (MI-FGSM's momentum); the legacy
    fused form would bake the capturing call's buffers into its graph, so such attacks stay eager under it."""
    from .. import hip_ops
    ops = attack.ops
    fused = fused_form()
    # launch profiling: brackets around kernels of the model part need eager launches; brackets around the step kernels only
    # (start_profile(..., graph_ok=True): bench.py's timed region) go with the split form, whose steps are plain launches
    profiling_allows = hip_ops._profile is None or (hip_ops._profile_graph_ok and not fused)
    use_graph = (enabled() and not attack._graph_off and ops is hip_ops and profiling_allows and adv.is_cuda and steps >= 4
                 and not torch.cuda.is_current_stream_capturing() and not (fused and step_has_state))
    done = 0
    if use_graph:
        # family: what makes two calls the same workload and may come back (train/eval flags and the ADVSTEP_* switches the
        # kernels read at call time included); state: parameter / buffer storage and versions, which never come back
        # ... and the launch stream: a capture serves ONE batch at a time (its static buffers, its activation pool), so two
        # streams with a batch in flight each (evaluation.generate_attacks) hold a capture each
        versions, buffers, flags = _state_signature(attack.model)
        family = (id(attack.model), attack.__class__.__name__, hyper, attack._targeted, tuple(adv.shape), str(adv.device),
                  labels.dtype, tuple(labels.shape), torch.cuda.current_stream(adv.device).cuda_stream, fused, flags, _toggles())
        key = family + ((versions, buffers),)
        _watch(attack.model)
        cap = _GRAPHS.get(key)
        if cap is None and family not in _FAILED:
            _SEEN[key] = _SEEN.get(key, 0) + 1
            if len(_SEEN) > 64:
                _SEEN.clear()
            if _SEEN.get(key, 0) >= 2:
                # a capture of this family under ANOTHER state can never be replayed again once the state moved on (training
                # changed the weights or the running statistics): drop it now — each holds a private pool with the whole
                # forward + backward activation set
                for stale in [k for k in _GRAPHS if k[:len(family)] == family]:
                    del _GRAPHS[stale]
                for stale in [k for k in _SEEN if k[:len(family)] == family and k != key]:
                    del _SEEN[stale]
                try:
                    cap = _Captured(attack, images, labels, target, step_fn, fused, step_has_state)
                    if len(_GRAPHS) >= _MAX_GRAPHS:
                        _GRAPHS.pop(next(iter(_GRAPHS)))
                    _GRAPHS[key] = cap
                except Exception as exc:  # noqa: BLE001 — any capture problem means: this workload stays eager, loudly
                    _FAILED.add(family)
                    torch.cuda.synchronize()
                    warnings.warn(f"hipGraph capture of the {attack.__class__.__name__} iteration failed ({exc!r}); "
                                  "continuing with eager launches for this workload")
                    cap = None
        if cap is not None:
            adv = cap.run(adv, images, labels, target, steps // 2, step_fn).detach().clone()
            done = 2 * (steps // 2)
    spare = None
    for _ in range(steps - done):
        grad, _ = attack._input_gradient(adv, labels, target)
        out = spare if spare is not None else torch.empty_like(adv)
        step_fn(adv.detach(), grad, images, out)
        spare, adv = adv.detach(), out
    return adv.detach()


def clear() -> None:
    """Drop every captured graph (tests; also releases the graphs' private memory pools)."""
    _GRAPHS.clear()
    _SEEN.clear()
    _FAILED.clear()
    for fin in list(_WATCHED.values()):
        fin.detach()
    _WATCHED.clear()
