"""k-means clustering (EM + kmeans++/random init), single- and multi-GPU.

Reference parity: RAFT's historical kmeans (balanced init + EM update built on
pairwise distance + argmin + reduce_rows_by_key + allreduce) — BASELINE
config 3: fit 10M x 256 fp32, k=1024, 8 MI355X over RCCL/xGMI.

MI355X design:
  * assignment step = fused L2-NN (distance tile + argmin, registers only;
    split-bf16 MFMA for the dot-product term on fp32 data),
  * update step = keyed row sums over the label-sorted rows (register
    accumulation per key run, atomics only at run boundaries) with the counts
    and the inertia folded into the same pass; the verified engines also
    refine every chosen distance in exact fp32 there,
  * distributed: rows are sharded across ranks (one process per GPU); per-iter
    global state is ONE allreduce of the [k, d+2] packed (sums | counts |
    inertia) buffer — a few MB over xGMI. Large shards split their rows in
    two halves so one half's allreduce hides under the other's compute.
"""
from __future__ import annotations

import functools
import math
import os
from dataclasses import dataclass, replace

import torch

from raft_amd._ext import require_ext
from raft_amd.comms import Comms, LoopbackComms, ReduceOp
from raft_amd.distance import pairwise_distance
from raft_amd.linalg.reduce_by_key import reduce_rows_by_key
from raft_amd.linalg.split_bf16 import (SPLIT_BOUND, VERIFY_MODES, pad_features,
                                        split_bf16_slices)
from raft_amd.matrix.sample_rows import sample_rows
from raft_amd.neighbors.fused_l2nn import (FUSED_NSLICE, fused_l2nn,
                                           fused_l2nn_presplit)
from raft_amd.random.rng import RngState, sample_without_replacement, uniform


@dataclass
class KMeansParams:
    n_clusters: int = 8
    max_iter: int = 20
    tol: float = 1e-4
    seed: int = 0
    init: str = "kmeans++"      # "kmeans++" | "scalable" (kmeans||) | "random" | "array"
    n_init: int = 1             # restarts with derived seeds; best inertia wins
    oversampling: float = 2.0   # kmeans||: l = oversampling * k samples/round
    fp32_mode: str = "auto"     # GEMM engine for the assignment step
    verbose: bool = False


@dataclass
class KMeansModel:
    centroids: torch.Tensor
    inertia: float
    n_iter: int
    labels: torch.Tensor | None = None


def _init_random(x: torch.Tensor, k: int, state: RngState, comms: Comms) -> torch.Tensor:
    """Sample k rows globally: each rank samples, rank-0's choice wins via bcast."""
    n_local = x.shape[0]
    idx = sample_without_replacement(n_local, min(k, n_local), state=state, device=x.device)
    cand = x[idx]
    if comms.get_size() > 1:
        # gather candidates from all ranks then keep k (deterministic: sorted by rank)
        all_c = comms.allgather(cand[: max(1, k // comms.get_size() + 1)])
        cand = all_c.reshape(-1, x.shape[1])[:k].contiguous()
        cand = comms.bcast(cand, root=0)
    return cand[:k].clone()


def _init_plusplus(x: torch.Tensor, k: int, state: RngState, comms: Comms,
                   fp32_mode: str,
                   sample_weights: torch.Tensor | None = None) -> torch.Tensor:
    """Greedy k-means++ (weighted D^2 sampling with local trials), distributed-aware.

    Reference parity: the reference's kmeansPlusPlus (and sklearn) draw
    2+log(k) candidates per step by D^2 and keep the one that minimizes the
    resulting potential — pure sequential D^2 misses a blob with measurable
    probability at large k; greedy selection drives that to ~0. With
    sample_weights (the kmeans|| candidate-reduction path), both the D^2
    sampling CDF and the candidate potentials are weighted by w, matching the
    reference's initScalableKMeansPlusPlus ownership weighting.

    Each step: every rank holds min-sq-distances to chosen centers for its
    shard; ranks compute local (weighted) D^2 sums, candidates are sampled
    rank/row proportionally and broadcast; candidate potentials are computed
    from one [n_local, L] GEMM-shaped distance block and allreduced.
    """
    n_local, d = x.shape
    world = comms.get_size()
    rank = comms.get_rank()
    w = None if sample_weights is None else sample_weights.double().clamp_min(0)
    n_trials = 2 + int(math.log(max(2, k)))
    # first center: global row 0 owner = rank 0 (deterministic from seed)
    u = uniform((1,), state=state, device=x.device)
    first = int((u.item() * n_local)) % n_local
    c0 = x[first:first + 1].clone()
    if world > 1:
        c0 = comms.bcast(c0, root=0)
    centers = [c0[0]]
    mind2 = fused_l2nn(x, c0, fp32_mode=fp32_mode)[0].double()
    xsq = (x * x).sum(dim=1)
    for _ in range(1, k):
        wd2 = mind2 if w is None else mind2 * w
        local_sum = wd2.sum()
        if world > 1:
            sums = comms.allgather(local_sum.reshape(1)).reshape(-1)
        else:
            sums = local_sum.reshape(1)
        total = float(sums.sum().item())
        cdf = torch.cumsum(wd2, dim=0)
        if world == 1:
            # vectorized trial sampling: ONE uniform draw + ONE searchsorted
            # for all L candidates (the per-trial .item() loop costs ~2
            # host syncs x k x L on GPU — ~12k syncs at k=1024)
            us = uniform((n_trials,), state=state, device=x.device).double() * total
            js = torch.searchsorted(cdf, us.to(cdf.dtype)).clamp_(max=n_local - 1)
            cmat = x[js]                                       # [L, d]
        else:
            cands = []
            for t in range(n_trials):
                u = float(uniform((1,), state=state, device=x.device).item()) * total
                # pick owning rank by prefix sums
                csum = 0.0
                owner, local_u = 0, u
                for r in range(world):
                    s = float(sums[r].item())
                    if u < csum + s or r == world - 1:
                        owner, local_u = r, u - csum
                        break
                    csum += s
                if rank == owner:
                    j = int(torch.searchsorted(cdf, torch.tensor(local_u, dtype=cdf.dtype,
                                                                 device=cdf.device)).item())
                    j = min(j, n_local - 1)
                    cand = x[j:j + 1].clone()
                else:
                    cand = torch.empty((1, d), dtype=x.dtype, device=x.device)
                cands.append(comms.bcast(cand, root=owner)[0])
            cmat = torch.stack(cands, dim=0)                   # [L, d]
        center, mind2 = _keep_best_candidate(x, xsq, cmat, mind2, w, comms)
        centers.append(center)
    return torch.stack(centers, dim=0)


def _keep_best_candidate(x, xsq, cmat, mind2, w, comms):
    """One greedy k-means++ selection: of the candidate rows cmat [L, d], keep
    the one that minimizes the (weighted, global) potential. Returns it with
    the min-sq-distances updated for it."""
    # [n_local, L] squared distances in fp32 (no fp64 copy of x):
    # ||x||^2 + ||c||^2 - 2 x.c — selection only needs ~1e-7 relative
    d2 = (xsq.unsqueeze(1) + (cmat * cmat).sum(dim=1)
          - 2.0 * (x @ cmat.T)).clamp_min_(0).double()
    pot = torch.minimum(mind2.unsqueeze(1), d2)                 # [n_local, L]
    pot = (pot if w is None else pot * w.unsqueeze(1)).sum(dim=0)  # [L]
    if comms.get_size() > 1:
        comms.allreduce(pot, op=ReduceOp.SUM)
    best = int(pot.argmin().item())
    return cmat[best], torch.minimum(mind2, d2[:, best])


def _init_scalable(x: torch.Tensor, k: int, state: RngState, comms: Comms,
                   fp32_mode: str, oversampling: float = 2.0,
                   n_rounds: int = 5) -> torch.Tensor:
    """kmeans|| (scalable k-means++), distributed-aware.

    Reference parity: the reference's initScalableKMeansPlusPlus — instead of
    k sequential D^2 draws (k synchronization points), do ~5 rounds that each
    sample l = oversampling*k points INDEPENDENTLY with probability
    min(1, l*d2/total), then weight the ~l*rounds candidates by how many
    points they own and reduce them to k centers with (weighted) k-means++ +
    a few Lloyd steps on the tiny candidate set.
    """
    n_local, d = x.shape
    world = comms.get_size()
    l = max(int(oversampling * k), 2)
    # first center (rank 0's draw wins)
    u = uniform((1,), state=state, device=x.device)
    j0 = int(u.item() * n_local) % n_local
    c0 = x[j0:j0 + 1].clone()
    if world > 1:
        c0 = comms.bcast(c0, root=0)
    cands = [c0]
    mind2 = fused_l2nn(x, c0, fp32_mode=fp32_mode)[0]
    for _ in range(n_rounds):
        total = mind2.sum().reshape(1)
        if world > 1:
            comms.allreduce(total, op=ReduceOp.SUM)
        tot = float(total.item())
        if tot <= 0:
            break
        p = (mind2 * (l / tot)).clamp_(max=1.0)
        draw = uniform((n_local,), state=state, device=x.device) < p
        new_c = x[draw]
        if world > 1:
            counts = torch.tensor([new_c.shape[0]], device=x.device)
            all_counts = comms.allgather(counts).reshape(-1)
            new_c = comms.allgatherv(new_c.reshape(new_c.shape[0], d),
                                     [int(c) for c in all_counts])
        if new_c.shape[0] == 0:
            continue
        cands.append(new_c)
        nd2 = fused_l2nn(x, new_c, fp32_mode=fp32_mode)[0]
        mind2 = torch.minimum(mind2, nd2)
    cand = torch.cat(cands, dim=0)          # identical on every rank
    # weight candidates by ownership over the (global) data
    _, owner = fused_l2nn(x, cand, fp32_mode=fp32_mode)
    w = torch.bincount(owner, minlength=cand.shape[0]).to(x.dtype)
    if world > 1:
        comms.allreduce(w, op=ReduceOp.SUM)
    if cand.shape[0] <= k:
        # degenerate: too few candidates — pad with random rows
        extra = _init_random(x, k - cand.shape[0], state, comms)
        return torch.cat([cand, extra], dim=0)[:k]
    # cluster the candidates: weighted k-means++ seeding + weighted Lloyd
    sub = kmeans_fit(cand, KMeansParams(n_clusters=k, max_iter=10,
                                        seed=state.seed ^ 0x5bd1e995,
                                        init="kmeans++", fp32_mode=fp32_mode),
                     sample_weights=w)
    return sub.centroids


def kmeans_fit(x: torch.Tensor, params: KMeansParams,
               comms: Comms | None = None,
               init_centroids: torch.Tensor | None = None,
               sample_weights: torch.Tensor | None = None) -> KMeansModel:
    """Lloyd EM. `x` is THIS RANK's row shard; pass comms for multi-GPU.

    sample_weights: optional per-row weights (reference kmeans API parity) —
    weighted centroid updates and weighted inertia.

    n_init > 1 (reference kmeans_types n_init): run the whole fit n_init
    times with derived seeds and keep the lowest-inertia model — the
    standard guard against kmeans++ local optima. Seeds are derived
    deterministically so every rank replays the same trials.
    """
    if params.n_init > 1 and init_centroids is None and params.init != "array":
        best = None
        for trial in range(params.n_init):
            p = replace(params, n_init=1, seed=params.seed + 9973 * trial)
            m = kmeans_fit(x, p, comms, None, sample_weights)
            if best is None or m.inertia < best.inertia:
                best = m
        return best
    comms = comms or LoopbackComms()
    state = RngState(seed=params.seed)
    k, d = params.n_clusters, x.shape[1]

    if init_centroids is not None or params.init == "array":
        centroids = init_centroids.to(x.device, x.dtype).clone()
    elif params.init == "random":
        centroids = _init_random(x, k, state, comms)
    elif params.init in ("scalable", "kmeans||"):
        centroids = _init_scalable(x, k, state, comms, params.fp32_mode,
                                   oversampling=params.oversampling)
    else:
        centroids = _init_plusplus(x, k, state, comms, params.fp32_mode,
                                   sample_weights=sample_weights)

    nslice = _fused_nslice(x, params.fp32_mode, d)
    if nslice is not None:
        # X is iteration-invariant: split it once, not once per assignment
        x_slices = split_bf16_slices(x, nslice)
        xn = (x * x).sum(dim=1)
        vx = x if params.fp32_mode in VERIFY_MODES else None
        assign = functools.partial(fused_l2nn_presplit, x_slices, xn, verify_x=vx)
    else:
        assign = functools.partial(fused_l2nn, x, fp32_mode=params.fp32_mode)

    inertia = float("inf")
    it = 0
    labels = None
    for it in range(1, params.max_iter + 1):
        new_centroids, counts, inertia_t, dmin, labels = _lloyd_step(
            x, centroids, assign, comms, sample_weights)
        inertia = float(inertia_t.item())
        # empty clusters: relocate to the globally farthest point (reference
        # relocates empties; here: owner rank = argmax of local max-dmin)
        empties = (~(counts > 0)).nonzero(as_tuple=True)[0]
        if empties.numel():
            used = set()
            order = torch.argsort(dmin, descending=True)
            for ci in empties.tolist():
                local_best = None
                for cand in order[: len(used) + 1].tolist():
                    if cand not in used:
                        local_best = cand
                        break
                used.add(local_best)
                lv = float(dmin[local_best].item())
                if comms.get_size() > 1:
                    vals = comms.allgather(torch.tensor([lv], device=x.device,
                                                        dtype=torch.float32)).reshape(-1)
                    owner = int(vals.argmax().item())
                    row = x[local_best:local_best + 1].clone() if owner == comms.get_rank() \
                        else torch.empty((1, d), dtype=x.dtype, device=x.device)
                    row = comms.bcast(row, root=owner)
                    new_centroids[ci] = row[0]
                else:
                    new_centroids[ci] = x[local_best]
        shift = float(((new_centroids - centroids) ** 2).sum().item())
        centroids = new_centroids
        if params.verbose:
            print(f"[kmeans] iter {it} inertia {inertia:.4e} shift {shift:.3e}")
        if shift <= params.tol * params.tol:
            break
    return KMeansModel(centroids=centroids, inertia=inertia, n_iter=it, labels=labels)


def _accum_dtype(dtype: torch.dtype) -> torch.dtype:
    """Sums, counts and inertia of half-precision data accumulate in fp32: bf16
    holds no count > 256 exactly, which corrupts the centroids of large clusters."""
    return torch.float32 if dtype in (torch.bfloat16, torch.float16) else dtype


def _lloyd_step(x, centroids, assign, comms, sample_weights=None):
    """One generic Lloyd step on this rank's shard. assign(centroids) gives
    (dmin, labels); sums by key, counts and the inertia then travel in ONE
    packed allreduce. Returns (new centroids, counts, inertia, dmin, labels);
    the inertia stays a device scalar, so the caller decides when to sync."""
    k, d = centroids.shape
    dmin, labels = assign(centroids)
    acc = _accum_dtype(x.dtype)
    if sample_weights is None:
        sums = reduce_rows_by_key(x, labels, n_keys=k, out_dtype=acc)
        counts = torch.bincount(labels, minlength=k).to(acc)
        local_inertia = torch.sum(dmin, dtype=torch.float64).to(acc)
    else:
        w = sample_weights.to(acc)
        sums = reduce_rows_by_key(x, labels, n_keys=k, weights=w, out_dtype=acc)
        counts = torch.zeros(k, dtype=acc, device=x.device)
        counts.index_add_(0, labels.to(torch.int64), w)
        local_inertia = torch.sum(dmin.to(acc) * w, dtype=torch.float64).to(acc)
    # [k, d] sums | [k] counts | [1] inertia
    packed = torch.cat([sums.reshape(-1), counts, local_inertia.reshape(1)])
    if comms.get_size() > 1:
        comms.allreduce(packed, op=ReduceOp.SUM)
    sums = packed[: k * d].reshape(k, d)
    counts = packed[k * d: k * d + k]
    # sums / counts where a cluster has members, the old centroid elsewhere
    # (no boolean indexing: that would sync the host every step)
    nonzero = counts > 0
    mean = sums / torch.where(nonzero, counts, torch.ones_like(counts)).unsqueeze(1)
    new_centroids = torch.where(nonzero.unsqueeze(1), mean.to(x.dtype), centroids)
    return new_centroids, counts, packed[-1], dmin, labels


#: slices "auto" starts on: the adaptive loop runs the 1-product engine first
#: and widens to the mode's 2 slices if too many rows would rescan
_AUTO_START_NSLICE = 1
#: columns the widest kmeans_update_verify kernel instance covers (16 per lane)
_UPDATE_VERIFY_MAX_D = 1024


def _fused_nslice(x: torch.Tensor, fp32_mode: str, d: int):
    """Slices of the mode if fp32 data of (padded) width d takes the fused
    route (presplit X; in kmeans_iterate the minimal-dispatch loop), else None.
    A verified mode wider than its update kernel covers takes the generic loop,
    whose verify/repair and keyed reduction are written for any d."""
    fused = (x.is_cuda and x.dtype == torch.float32 and fp32_mode in FUSED_NSLICE
             and d % 64 == 0
             and not (fp32_mode in VERIFY_MODES and d > _UPDATE_VERIFY_MAX_D))
    return FUSED_NSLICE[fp32_mode] if fused else None


class KMeansIterState:
    """Iteration-invariant operands of one X shard: bf16 slices and row norms.
    Made by kmeans_iter_state and passed to kmeans_iterate as state=; slices
    that one call adds stay for the next."""

    def __init__(self, x: torch.Tensor, nslice: int):
        self.x = x.contiguous()
        self.slices = []
        self.xn = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        self.ensure(nslice)

    def ensure(self, nslice: int) -> None:
        """Make sure nslice slices exist. One fused pass writes all of them
        and xn; slices that existed already get identical values again."""
        if len(self.slices) < nslice:
            self.slices += [torch.empty_like(self.x, dtype=torch.bfloat16)
                            for _ in range(nslice - len(self.slices))]
            require_ext().split_bf16_norms(self.x, self.slices, self.xn)


def kmeans_iter_state(x: torch.Tensor, fp32_mode: str = "auto"):
    """Precompute the iteration-invariant inputs (bf16 slices of X + row
    norms) ONCE per fit — reusable across kmeans_iterate calls. On GPU this
    is a single fused kernel pass (ext.split_bf16_norms). None where
    kmeans_iterate takes the generic loop."""
    nslice = _fused_nslice(x, fp32_mode, x.shape[1])
    if nslice is None:
        return None
    # "auto" starts on the 1-product engine: only slice 0 here (half the split
    # memory and pass); the adaptive loop adds the residual slice if it widens
    return KMeansIterState(x, _AUTO_START_NSLICE if fp32_mode == "auto" else nslice)


def kmeans_iterate(x: torch.Tensor, centroids: torch.Tensor, n_iters: int,
                   comms: Comms | None = None, fp32_mode: str = "auto",
                   chunk_rows: int = 262144, state=None):
    """Run EXACTLY n_iters Lloyd iterations (no convergence early-exit).

    The benchmark entry point: every iteration performs the full assignment
    (fused L2-NN over all rows) + update (keyed reduction, counts, ONE packed
    allreduce, centroid recompute). Returns (centroids, inertia).
    """
    comms = comms or LoopbackComms()
    d = centroids.shape[1]
    if d % 64 and _fused_nslice(x, fp32_mode, d + (-d) % 64) is not None:
        # zero feature columns change nothing (distances, sums, counts all
        # identical; padded centroid columns stay 0): pad to the MFMA K
        # granularity so ANY d takes the fused engines
        c_out, inertia = kmeans_iterate(pad_features(x), pad_features(centroids),
                                        n_iters, comms=comms, fp32_mode=fp32_mode,
                                        chunk_rows=chunk_rows)
        return c_out[:, :d].contiguous(), inertia
    if _fused_nslice(x, fp32_mode, d) is not None:
        # X is iteration-invariant: pre-split the bf16 slices and row norms
        # ONCE (the same caching the reference does for row norms)
        ops = state if state is not None else kmeans_iter_state(x, fp32_mode)
        assert ops.x.shape == x.shape, "state= was made for another X"
        return _FastLoop(ops, centroids.contiguous().clone(), comms,
                         fp32_mode).run(n_iters)
    assign = functools.partial(fused_l2nn, x, fp32_mode=fp32_mode,
                               chunk_rows=chunk_rows)
    inertia_t = None
    for _ in range(n_iters):
        centroids, _, inertia_t, _, _ = _lloyd_step(x, centroids, assign, comms)
    # single host sync at the end (a per-iter .item() serializes the pipeline)
    inertia = float(inertia_t.item()) if inertia_t is not None else float("inf")
    return centroids, inertia


#: engine chosen by the last adaptive (fp32_mode="auto") _FastLoop run
#: (1 = stayed on bf16x1v, 2 = widened to bf16x2v) — test observability
_LAST_ADAPTIVE_NSLICE = None


class _FastLoop:
    """Minimal-dispatch EM loop: every per-iteration stage is ONE kernel
    (centroid split+norms, fused assignment, verify/repair, keyed reduction
    with counts, centroid update) + the rocPRIM label sort + ONE packed
    allreduce.

    Multi-GPU (world > 1): SPLIT-BATCH overlap (VERDICT r1 item 8 /
    SURVEY §6) — local rows are split in two halves; half A's packed
    allreduce is issued async (it runs on RCCL's communicator stream) while
    half B's assignment+reduction kernels execute on the compute stream, so
    the collective hides under compute. allreduce(A)+allreduce(B) equals
    allreduce(A+B) by linearity, so the update is bitwise the same modulo
    fp32 summation order. Opt out with RAFT_AMD_KMEANS_OVERLAP=0.

    fp32_mode="auto" is adaptive: start on the 1-product bf16x1v engine
    (1/3 the MFMA work), measure the provable-rescan fraction of the FIRST
    iteration (rows whose emulated margin falls inside the wide 2^-7 bound),
    and widen to the 2-slice engine if >2% of rows would rescan. Both
    engines produce the exact fp32 argmin, so the switch is purely a
    performance guard — per-rank decisions need not agree.
    """

    def __init__(self, ops: KMeansIterState, centroids, comms, fp32_mode):
        self.ext = require_ext()
        self.ops, self.comms = ops, comms
        self.k, self.d = centroids.shape
        self.verify = fp32_mode in VERIFY_MODES
        self.adaptive = fp32_mode == "auto"
        # slices of the mode, and of the engine in use: "auto" starts narrower
        self.nslice = FUSED_NSLICE[fp32_mode]
        self.cur_nslice = _AUTO_START_NSLICE if self.adaptive else self.nslice
        ops.ensure(self.cur_nslice)
        #: first-iteration provable-rescan fraction (device scalar)
        self.rescan_frac = None
        # ANY k takes this path: pad the centroid rows to a 128 multiple with
        # ZERO vectors whose cn entries are poisoned to +inf after each split —
        # the sweep can never pick them (score = inf), the verify/rescan kernels
        # see only the real k rows (centroids[:k] slice), and update leaves the
        # zero rows untouched (counts 0)
        self.kp = kp = self.k + (-self.k) % 128
        if kp > self.k:
            centroids = torch.cat([centroids, centroids.new_zeros(kp - self.k, self.d)])
        self.centroids = centroids
        self.c_slices = [centroids.new_empty((kp, self.d), dtype=torch.bfloat16)
                         for _ in range(self.nslice)]
        self.cn = centroids.new_empty(kp)
        self.cn_max = centroids.new_zeros(1)
        # overlap pays when the halves keep the GPU busy longer than the doubled
        # per-iteration dispatch (~0.5 ms) it costs — gate on shard size
        # (RAFT_AMD_KMEANS_OVERLAP=1 forces on, =0 off)
        n = ops.x.shape[0]
        ov_env = os.environ.get("RAFT_AMD_KMEANS_OVERLAP", "auto")
        self.overlap = (comms.get_size() > 1 and n >= 2
                        and (ov_env == "1" or (ov_env != "0" and n >= 4_000_000)))
        self._cut_row_ranges()

    def _cut_row_ranges(self):
        """(x, slices, xn) per row range: the two halves under overlap, else
        the whole shard. Cut again whenever ops gains a slice."""
        ops, h = self.ops, self.ops.x.shape[0] // 2
        cuts = [slice(0, h), slice(h, None)] if self.overlap else [slice(None)]
        self.row_ranges = [(ops.x[c], [s[c] for s in ops.slices], ops.xn[c])
                           for c in cuts]

    def _split_centroids(self):
        self.ext.split_bf16_norms(self.centroids, self.c_slices[:self.cur_nslice],
                                  self.cn, self.cn_max)
        if self.kp > self.k:
            # poison the padding rows' norms AFTER the split (their zero
            # vectors leave the fused cn_max untouched): sweep score = +inf
            self.cn[self.k:].fill_(float("inf"))

    def _local_update(self, xh, xh_slices, xnh):
        """assignment + keyed reduction for one row range -> packed buffer"""
        ext, k, kp, d = self.ext, self.k, self.kp, self.d
        lead, tail = SPLIT_BOUND[self.cur_nslice]
        dmin, amin, dmin2 = ext.fused_l2nn_split(xh_slices[:self.cur_nslice],
                                                 self.c_slices[:self.cur_nslice],
                                                 xnh, self.cn)
        if self.adaptive and self.rescan_frac is None:
            # pre-repair margin stats (dmin is overwritten by the verify
            # kernel below): fraction of rows the exact rescan will touch
            b = 2.0 * (lead * (xnh * self.cn_max).clamp_min(0).sqrt()
                       + tail * (xnh + self.cn_max))
            self.rescan_frac = ((dmin2 - dmin) < b).float().mean()
        keys_sorted, perm = torch.sort(amin)
        packed = torch.zeros(kp * d + kp + 1, dtype=torch.float32, device=xh.device)
        sums = packed[: kp * d].view(kp, d)
        counts = packed[kp * d: kp * d + kp]
        if self.verify:
            # ONE X pass: centroid-sum accumulation + exact-fp32
            # verify/refine + the inertia fold (sum of the FINAL repaired
            # distances accumulates into packed[-1] in-kernel); cn_max comes
            # fused out of split_bf16_norms. centroids[:k]: the rescan must
            # only see the REAL rows (the zero padding rows would win it)
            ext.kmeans_update_verify(xh, perm.to(torch.int32), keys_sorted,
                                     self.centroids[:k], xnh, dmin, amin, dmin2,
                                     self.cn_max, sums, counts, packed[-1:],
                                     lead=lead, tail=tail)
        else:
            ext.reduce_rows_by_key_sorted_into(xh, perm.to(torch.int32), keys_sorted,
                                               sums, counts, dmin, packed[-1:])
        return packed

    def _combine(self):
        """Every row range's packed buffer, summed over ranges and ranks."""
        comms = self.comms
        if not self.overlap:
            packed = self._local_update(*self.row_ranges[0])
            if comms.get_size() > 1:
                comms.allreduce(packed, op=ReduceOp.SUM)
            return packed
        packed_a = self._local_update(*self.row_ranges[0])
        work_a = comms.allreduce_async(packed_a, op=ReduceOp.SUM)
        packed_b = self._local_update(*self.row_ranges[1])
        work_b = comms.allreduce_async(packed_b, op=ReduceOp.SUM)
        for work in (work_a, work_b):
            if work is not None:
                work.wait()
        packed_a += packed_b
        return packed_a

    def _update_centroids(self, packed):
        kp, d = self.kp, self.d
        self.ext.kmeans_update_centroids(packed[: kp * d].view(kp, d),
                                         packed[kp * d: kp * d + kp],
                                         self.centroids)

    def _decide_widen(self):
        """Once, after the first adaptive iteration (one host sync): widen to
        the tight-bound 2-slice engine if the wide bf16x1v bound would rescan
        >2% of rows each iteration."""
        global _LAST_ADAPTIVE_NSLICE
        if self.nslice > self.cur_nslice and float(self.rescan_frac.item()) > 0.02:
            self.ops.ensure(self.nslice)
            self._cut_row_ranges()
            self.cur_nslice = self.nslice
        self.adaptive = False
        _LAST_ADAPTIVE_NSLICE = self.cur_nslice

    def run(self, n_iters):
        packed = None
        for _ in range(n_iters):
            self._split_centroids()
            packed = self._combine()
            self._update_centroids(packed)
            if self.adaptive:
                self._decide_widen()
        inertia = float(packed[-1].item()) if packed is not None else float("inf")
        return self.centroids[:self.k], inertia


def kmeans_predict(model_or_centroids, x: torch.Tensor, fp32_mode: str = "auto") -> torch.Tensor:
    """Assign each row of x to its nearest centroid (fused L2-NN argmin)."""
    c = getattr(model_or_centroids, "centroids", model_or_centroids)
    return fused_l2nn(x, c, fp32_mode=fp32_mode)[1]


def kmeans_transform(model_or_centroids, x: torch.Tensor, fp32_mode: str = "auto") -> torch.Tensor:
    """Distance of each row of x to every centroid ([n, k] matrix)."""
    c = getattr(model_or_centroids, "centroids", model_or_centroids)
    return pairwise_distance(x, c, fp32_mode=fp32_mode)


def kmeans_balanced_fit(x: torch.Tensor, n_clusters: int, max_iter: int = 20,
                        seed: int = 0, sample_fraction: float = 0.1,
                        fp32_mode: str = "auto") -> KMeansModel:
    """Balanced/hierarchical-flavored k-means (reference kmeans_balanced
    parity): train on a uniform subsample (the ANN-index-build usage), then
    assign the full set; clusters that end up empty are refilled from the
    largest cluster's farthest points, trading inertia for balance.
    """
    n = x.shape[0]
    n_sample = max(n_clusters * 4, int(n * sample_fraction))
    xs = sample_rows(x, n_sample, state=RngState(seed=seed)) if n_sample < n else x
    model = kmeans_fit(xs, KMeansParams(n_clusters=n_clusters, max_iter=max_iter,
                                        seed=seed, init="random",
                                        fp32_mode=fp32_mode))
    labels = kmeans_predict(model, x, fp32_mode=fp32_mode)
    counts = torch.bincount(labels, minlength=n_clusters)
    model.labels = labels
    model.inertia = float(fused_l2nn(x, model.centroids,
                                     fp32_mode=fp32_mode)[0].double().sum())
    # refill empty clusters from the largest cluster's members
    for ci in (counts == 0).nonzero(as_tuple=True)[0].tolist():
        big = int(counts.argmax())
        members = (labels == big).nonzero(as_tuple=True)[0]
        d = fused_l2nn(x[members], model.centroids[big:big + 1],
                       fp32_mode=fp32_mode)[0]
        far = members[int(d.argmax())]
        model.centroids[ci] = x[far]
        counts[big] -= 1
        counts[ci] += 1
    return model


class KMeans:
    """Estimator-style wrapper."""

    def __init__(self, n_clusters: int = 8, max_iter: int = 20, tol: float = 1e-4,
                 seed: int = 0, init: str = "kmeans++", n_init: int = 1,
                 oversampling: float = 2.0, fp32_mode: str = "auto",
                 verbose: bool = False):
        self.params = KMeansParams(n_clusters=n_clusters, max_iter=max_iter, tol=tol,
                                   seed=seed, init=init, n_init=n_init,
                                   oversampling=oversampling, fp32_mode=fp32_mode,
                                   verbose=verbose)
        self.model: KMeansModel | None = None

    def fit(self, x: torch.Tensor, comms: Comms | None = None) -> "KMeans":
        self.model = kmeans_fit(x, self.params, comms=comms)
        return self

    @property
    def cluster_centers_(self):
        return self.model.centroids

    @property
    def inertia_(self):
        return self.model.inertia

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        return kmeans_predict(self.model, x, fp32_mode=self.params.fp32_mode)

    def transform(self, x: torch.Tensor) -> torch.Tensor:
        return kmeans_transform(self.model, x, fp32_mode=self.params.fp32_mode)

    def fit_predict(self, x: torch.Tensor, comms: Comms | None = None) -> torch.Tensor:
        return self.fit(x, comms=comms).predict(x)

    def fit_transform(self, x: torch.Tensor, comms: Comms | None = None) -> torch.Tensor:
        return self.fit(x, comms=comms).transform(x)

    def score(self, x: torch.Tensor) -> float:
        """Negative inertia of x under the fitted centroids (sklearn convention)."""
        dmin, _ = fused_l2nn(x, self.model.centroids, fp32_mode=self.params.fp32_mode)
        return -float(torch.sum(dmin, dtype=torch.float64))

    @property
    def labels_(self):
        return self.model.labels

    @property
    def n_iter_(self):
        return self.model.n_iter
