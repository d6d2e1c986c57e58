"""The brute-force pose search (csrc/pose_search.hip, csrc/morton_sort.hip, csrc/bf_prune.hip and the host loop of
utils/eval_3D.py::brute_force_search) against a CPU oracle that restates one search operation for operation - and demands
BIT EQUALITY of the whole record: cd, index, acc, comp, six F-scores, and the `evaluated` / `scanned` counters.

pose_search.hip is compiled with -ffp-contract=off and every reduction in it has a fixed order, so the record is a pure
function of the inputs.  The oracle below is numpy (fmaf through eval_3D._fma32) with oracle/chamfer_ref.c for the
nearest-neighbour minima:
  str_order      zs_str_sort: three stable sorts on (group << 32) | ordered_bits(coordinate), str_plan / str_group restated
  stats / apply  pose_stats_kernel (double partial sums strided by 256, xor butterfly per wave, waves in order, the mean
                 rounded once, den in fp32) and Xform::apply
  partials       write_partial: per 512-query block (0 + s[t]) + s[t + 256], butterfly, waves in order; six counters
  Oracle.batch   pose_kill_kernel (kill_test on the first `done` block sums against min(best[0], best[12]) as they stood
                 before the batch; merge when 4 * killed <= count) and pose_finish_kernel (winner rule, counters)
  Oracle.search  the host loop: first batch, stable order of the lower bounds, batch_pruned in fp32, peek after 2 and 4
The lower bounds are an INPUT of the oracle (taken from the GPU); section D checks their rigour instead.

Sections: A the record at the launcher's thresholds (sub-tile, query block, candidate tile, stage ends, T == 64 / 65, the
first-batch edge, the batch clamp); B host-loop variants and the C ABI (ties, index_offset, best[12], the dead and merge
flags in the scratch, refusals); C zs_pose_pack and zs_str_sort alone; D lower bounds on off-centre / scaled / tiny clouds.
tests/test_pose_edge_refs.py is the CPU side: constants read from the source, branch accounting, soundness of the oracle.

The builders / references below run on the CPU alone (the CPU module imports them)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import chamfer_ref as C
from tests.test_gpu_eval_edges import _rs, same_bits
from zeroshape_amd.utils.eval_3D import _fma32          # numpy only: fmaf on float32 arrays, correctly rounded

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
THRESHOLDS = (0.005, 0.01, 0.02, 0.05, 0.1, 0.2)
THREADS, Q_PER_LANE, TILE, SUB, LEAF = 256, 2, 1024, 64, 64      # tests/test_pose_edge_refs.py reads them from the source
BLOCK = THREADS * Q_PER_LANE
STAGE_ENDS = (2, 6)
MAX_BATCH, MERGE_SLOT, DEAD_INTS, STAT, PART = 256, 256, 256 + 64, 16, 8
PLANT = 2345                                                     # the planted alignment: rotation index on the sphere
NN = ("cull", "pairs", "brute")


@pytest.fixture(autouse=True)
def _default_stages():
    if os.environ.get("ZS_POSE_STAGES"):
        pytest.skip("ZS_POSE_STAGES moves the stage ends the oracle restates (the library reads it once per process)")


def ceil_div(a, b):
    return (a + b - 1) // b


@functools.lru_cache(maxsize=None)
def sphere():
    """The 6,912 rotations, built on the CPU (the tests hand THESE bits to the GPU search) [6912,3,3] float32."""
    from zeroshape_amd.utils.camera import get_rotation_sphere
    return get_rotation_sphere(azim_sample=24, elev_sample=24, roll_sample=12, scales=[1.0], device="cpu").float().contiguous().numpy()


# =====================================================================================================
# the oracle
# =====================================================================================================
def ordered_bits(v):
    u = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _ceil_root(v, k):
    r = 1
    while r ** k < v:
        r += 1
    return r


def str_plan(n):
    leaves = ceil_div(n, LEAF)
    per = ceil_div(leaves, _ceil_root(leaves, 3))
    return n, per * LEAF, _ceil_root(per, 2)               # n, slab_points, max_strips


def str_group(plan, i, which):
    n, slab_points, max_strips = plan
    slab = i // slab_points
    if which == 1:
        return slab
    begin = slab * slab_points
    length = np.minimum(slab_points, n - begin)
    leaves = ceil_div(length, LEAF)
    strips = np.array([_ceil_root(int(v), 2) for v in leaves]) if np.ndim(leaves) else _ceil_root(int(leaves), 2)
    per = ceil_div(leaves, strips)
    return slab * max_strips + (i - begin) // (per * LEAF)


def str_order(points):
    """zs_str_sort's permutation: sorted = points[perm]."""
    p = np.ascontiguousarray(points, F32)
    n = len(p)
    plan, perm, pos = str_plan(n), np.arange(n), np.arange(n)
    for which in range(3):
        cur = p[perm]
        ok = np.isfinite(cur).all(1)
        lo = np.where(ok, ordered_bits(cur[:, which]), np.uint32(0xffffffff)).astype(np.uint64)
        hi = np.zeros(n, np.uint64) if which == 0 else str_group(plan, pos, which).astype(np.uint64)
        perm = perm[np.argsort((hi << np.uint64(32)) | lo, kind="stable")]
    return perm.astype(np.int32)


def wave_reduce(v):
    """[..., 256] -> [...]: the xor butterfly (32 .. 1) inside each wave of 64, then waves 0..3 in order; in v's type."""
    w = v.reshape(v.shape[:-1] + (THREADS // 64, 64))
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lanes ^ o]
    w = w[..., 0]
    s = w[..., 0]
    for k in range(1, THREADS // 64):
        s = s + w[..., k]
    return s


def rotate(p, R):
    """p [n,3], R [B,9] float32 -> three [B,n] float32: the fmaf chain of Xform::rotate."""
    x, y, z = (p[None, :, a] for a in range(3))
    r = [R[:, i:i + 1] for i in range(9)]
    shape = (len(R), len(p))
    full = lambda a: np.broadcast_to(a, shape)
    return tuple(_fma32(full(r[3 * a + 2]), full(z), _fma32(full(r[3 * a + 1]), full(y), r[3 * a] * x)) for a in range(3))


IDENTITY = np.eye(3, dtype=F32).reshape(1, 9)


def stats(p, R):
    """pose_stats_kernel on the caller's order: mean [B,3] (double sums, rounded once) and den [B], float32."""
    n = len(p)
    rot = rotate(p, R)
    rows = ceil_div(n, THREADS)
    mean = []
    for a in range(3):
        v = np.zeros((len(R), rows * THREADS), F64)
        v[:, :n] = rot[a]                                   # (a thread without a point adds nothing; + 0.0 is exact)
        v = v.reshape(len(R), rows, THREADS)
        acc = np.zeros((len(R), THREADS), F64)
        for r in range(rows):
            acc = acc + v[:, r]
        mean.append((wave_reduce(acc) / n).astype(F32))
    lx = (rot[0].max(1) - mean[0]) - (rot[0].min(1) - mean[0])
    ly = (rot[1].max(1) - mean[1]) - (rot[1].min(1) - mean[1])
    return np.stack(mean, 1), np.maximum(lx, ly) + F32(1e-7)


def apply(p, R, mean, den):
    """Xform::apply: (R p - mean) / den in fp32 -> [B,n,3]."""
    rot = rotate(p, R)
    return np.stack([(rot[a] - mean[:, a:a + 1]) / den[:, None] for a in range(3)], 2).astype(F32)


def normalize(p):
    mean, den = stats(p, IDENTITY)
    return apply(p, IDENTITY, mean, den)[0]


def block_partials(d, thr, bx):
    """write_partial for every 512-query block: squared minima d [B,nq] -> [B,bx,8] (rows of unused blocks zero)."""
    B, nq = d.shape
    nb = ceil_div(nq, BLOCK)
    s = np.zeros((B, nb * BLOCK), F32)
    s[:, :nq] = np.sqrt(d)
    live = (np.arange(nb * BLOCK) < nq).reshape(nb, Q_PER_LANE, THREADS)
    s = s.reshape(B, nb, Q_PER_LANE, THREADS)
    out = np.zeros((B, bx, PART), F32)
    out[:, :nb, 0] = wave_reduce((F32(0) + s[:, :, 0]) + s[:, :, 1])
    for i in range(6):
        hit = ((s < thr[i]) & live).astype(F32)
        out[:, :nb, 1 + i] = wave_reduce((F32(0) + hit[:, :, 0]) + hit[:, :, 1])
    return out


def new_record(bound=np.inf):
    rec = np.zeros(16, F32)
    rec[0], rec[12] = np.inf, bound
    rec.view(np.int32)[1] = 0x7fffffff
    return rec


def batch_pruned(lb0, rec):
    """batch_pruned() of the kernels, in fp32."""
    return bool(F32(lb0) * (F32(1.0) - F32(1e-3)) - F32(1e-6) > min(rec[0], rec[12]))


class Oracle(object):
    """One (prediction, ground truth) pair: the sorted clouds and, per rotation of `rotations`, the partial sums."""

    def __init__(self, pred, gt, rotations, thresholds=THRESHOLDS):
        self.pred, self.R = np.ascontiguousarray(pred, F32), np.ascontiguousarray(rotations, F32).reshape(-1, 9)
        self.gt_n = normalize(np.ascontiguousarray(gt, F32))
        self.n, self.m = len(self.pred), len(self.gt_n)
        self.bx = ceil_div(max(self.n, self.m), BLOCK)
        self.nb = (ceil_div(self.n, BLOCK), ceil_div(self.m, BLOCK))
        self.pred_s, self.gt_s = self.pred[str_order(self.pred)], self.gt_n[str_order(self.gt_n)]
        self.thr = np.array(list(thresholds) + [0.0] * (6 - len(thresholds)), F32)
        self.part = {}
        self.trace = []                                      # per evaluated batch: (count, killed at stage 1, merged, dead)

    def applied(self, index, points=None):
        R = self.R[np.atleast_1d(index)]
        mean, den = stats(self.pred, R)
        return apply(self.pred if points is None else points, R, mean, den)

    def partials(self, index):
        """[len(index), 2, bx, 8] float32; computed once per rotation."""
        todo = sorted(set(int(k) for k in index) - set(self.part))
        for lo in range(0, len(todo), 64):
            ks = todo[lo:lo + 64]
            a = self.applied(ks, self.pred_s)
            d1, d2, _, _ = C.chamfer_forward(a, np.broadcast_to(self.gt_s, (len(ks),) + self.gt_s.shape))
            p1, p2 = block_partials(d1, self.thr, self.bx), block_partials(d2, self.thr, self.bx)
            for j, k in enumerate(ks):
                self.part[k] = np.stack([p1[j], p2[j]])
        return np.stack([self.part[int(k)] for k in index])

    def cd_of(self, index):
        return np.array([self.metrics(p)[0] for p in self.partials(index)], F32)

    def _sum(self, rows, done):
        s = np.zeros(rows.shape[:-1], F32)
        for b in range(done):
            s = s + rows[..., b]
        return s

    def kill_stat(self, P, done):
        """kill_test's left side per rotation: P [count,2,bx,8]."""
        s0 = self._sum(P[:, 0, :, 0], min(done, self.nb[0])) / F32(self.n)
        s1 = self._sum(P[:, 1, :, 0], min(done, self.nb[1])) / F32(self.m)
        return (s0 + s1) / F32(2)

    def metrics(self, P):
        """pose_finish_kernel's per-rotation part: P [2,bx,8] -> (cd, acc, comp, f[6])."""
        tot = [self._sum(P[d].T, self.nb[d]) for d in range(2)]        # [8] each, blocks in order
        acc, comp = tot[0][0] / F32(self.n), tot[1][0] / F32(self.m)
        cd = (acc + comp) / F32(2)
        with np.errstate(invalid="ignore", divide="ignore"):
            pr, rc = tot[0][1:7] / F32(self.n), tot[1][1:7] / F32(self.m)
            f = F32(2) * pr * rc / (pr + rc)
        f = np.where(np.isnan(f), F32(0), f).astype(F32)
        return (F32(np.inf) if np.isnan(cd) else cd), acc, comp, f

    def batch(self, rec, index, gidx, lb0=None):
        """One zs_pose_search_batch_sorted call: rotations self.R[index], reported as `gidx`; rec is updated in place.
        Returns the dead flags (None when the lower bound prunes the batch)."""
        count = len(index)
        if count == 0 or (lb0 is not None and batch_pruned(lb0, rec)):
            return None
        P = self.partials(index)
        bound = min(rec[0], rec[12])
        dead, merged, killed1 = np.zeros(count, bool), None, 0
        for stage, done in enumerate(STAGE_ENDS):
            if done < self.bx:
                dead |= self.kill_stat(P, done) > bound
                if stage == 0:
                    killed1 = int(dead.sum())
                    merged = 4 * killed1 <= count
        self.trace.append((count, killed1, merged, int(dead.sum())))
        best = (F32(np.inf), 0x7fffffff, None)
        for j in range(count):
            cd, acc, comp, f = (F32(np.inf), F32(0), F32(0), np.zeros(6, F32)) if dead[j] else self.metrics(P[j])
            if cd < best[0] or (cd == best[0] and int(gidx[j]) < best[1]):
                best = (cd, int(gidx[j]), (acc, comp, f))
        irec = rec.view(np.int32)
        irec[10] += count
        irec[11] += count - int(dead.sum())
        if best[0] < rec[0] or (best[0] == rec[0] and best[1] < irec[1]):
            rec[0], irec[1], rec[2], rec[3] = best[0], best[1], best[2][0], best[2][1]
            rec[4:10] = best[2][2]
        self.merged = merged
        return dead

    def search(self, start, stop, batch_size=256, first_batch=None, prune=True, peek=True, lb=None):
        """brute_force_search's host loop over rotations start .. stop - 1 -> the 16-word record.  `lb`: the GPU's lower
        bounds of that slice (needed when prune and the slice exceeds a batch)."""
        batch_size = min(int(batch_size), MAX_BATCH)
        first_batch = min(batch_size, 32) if first_batch is None else max(1, min(int(first_batch), batch_size))
        K = stop - start
        order = lb_sorted = None
        if prune and K > batch_size:
            order = np.argsort(lb, kind="stable")
            lb_sorted = lb[order]
        rec, pos, bi = new_record(), 0, 0
        while pos < K:
            count = min(first_batch if pos == 0 else batch_size, K - pos)
            if peek and lb_sorted is not None and bi in (2, 4) and batch_pruned(lb_sorted[pos], rec):
                break
            if order is not None:
                self.batch(rec, start + order[pos:pos + count], start + order[pos:pos + count], lb_sorted[pos])
            else:
                self.batch(rec, np.arange(start + pos, start + pos + count), np.arange(start + pos, start + pos + count))
            pos, bi = pos + count, bi + 1
        return rec


def pack_ref(p):
    """zs_pose_pack's buffer: [sub-tile][x|y|z][64] (+inf padded) | [sub-tile] lo[3], hi[3], 0, 0 | [tile] the same."""
    p = np.ascontiguousarray(p, F32)
    n = len(p)
    ns = ceil_div(n, TILE) * (TILE // SUB)
    c = np.full((ns * SUB, 3), np.inf, F32)
    c[:n] = p
    c = c.reshape(ns, SUB, 3)
    live = (np.arange(ns * SUB) < n).reshape(ns, SUB, 1) & np.isfinite(c)
    box = np.zeros((ns, 8), F32)
    box[:, 0:3] = np.where(live, c, F32(np.inf)).min(1)
    box[:, 3:6] = np.where(live, c, F32(-np.inf)).max(1)
    tiles = box.reshape(ns // 16, 16, 8)
    tbox = np.zeros((ns // 16, 8), F32)
    tbox[:, 0:3], tbox[:, 3:6] = tiles[:, :, 0:3].min(1), tiles[:, :, 3:6].max(1)
    return np.concatenate([c.transpose(0, 2, 1).ravel(), box.ravel(), tbox.ravel()])


# =====================================================================================================
# clouds
# =====================================================================================================
KINDS = ("aligned", "unalignable", "flat", "two_clusters", "lattice", "duplicates", "offset")


@functools.lru_cache(maxsize=None)
def clouds(n, m, kind, seed=0):
    """(pred [n,3], gt [m,3]) float32.  Except for `unalignable`, pred = R[PLANT]^T (the shape) + 2e-3 noise."""
    rs = _rs(7, n, m, KINDS.index(kind), seed)
    big = max(n, m)
    if kind == "unalignable":
        e = rs.randn(n, 3)
        # (nearly a sphere: every rotation's cd is within a few per cent of the best, so no partial sum exceeds it)
        pred = e / np.linalg.norm(e, axis=1, keepdims=True) * np.array([0.5, 0.49, 0.48])
        return pred.astype(F32), rs.uniform(-0.5, 0.5, (m, 3)).astype(F32)
    if kind == "two_clusters":
        pool = rs.randn(big, 3) * 0.1 + np.where(rs.rand(big, 1) < 0.5, -5.0, 5.0) * np.array([1.0, 0.3, 0.0])
    elif kind == "lattice":
        g = np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing="ij"), -1).reshape(-1, 3) / 8.0 * np.array([1.0, 0.7, 0.5])
        pool = g[rs.permutation(big) % len(g)]
    elif kind == "duplicates":
        base = rs.randn(ceil_div(big, 7), 3) * np.array([0.5, 0.3, 0.2])
        pool = np.repeat(base, 7, axis=0)[:big][rs.permutation(big)]
    else:
        pool = rs.randn(big, 3) * np.array([0.5, 0.3, 0.2]) + rs.rand(big, 1) * 0.3
    if kind == "flat":
        pool[:, 2] = 0.0
    R = sphere()[PLANT].astype(F64)
    if big > 65536:
        # The T cases: tile 64 of the long cloud holds ONE point, the last of its STR order.  It is an outlier beyond the +x,
        # +y, +z corner of the long cloud's own frame, and both clouds hold it: each one's nearest neighbour in the other
        # cloud, so a walk that never reaches tile 64 changes a minimum (last_tile_matters(), asserted on the CPU).
        corner = np.array([6.0, 5.0, 4.0])
        pool[0] = corner if m > n else corner @ R.T
    gt = pool[:m]
    pred = pool[:n] @ R + (2e-3 * rs.randn(n, 3) if kind not in ("lattice", "duplicates") else 0.0)   # rows: R^T p
    if kind == "flat":
        gt = gt.copy()                                       # (the noise must not lift the ground truth off its plane)
    if kind == "offset":
        ext = float(np.ptp(pool, axis=0).max())
        pred, gt = pred + 100.0 * ext * np.array([1.0, -1.0, 0.5]), gt + 100.0 * ext * np.array([-1.0, 0.5, 1.0])
    return np.ascontiguousarray(pred, F32), np.ascontiguousarray(gt, F32)


def case(n, m, kind="aligned", lo=PLANT - 10, hi=PLANT + 22, **kw):
    return (n, m, kind, lo, hi, tuple(sorted(kw.items())))


def case_id(c):
    return "%dx%d-%s-%d+%d%s" % (c[0], c[1], c[2], c[3], c[4] - c[3], "".join("-%s%s" % kv for kv in c[5]))


SMALL = [(1, 1), (1, 7), (5, 3), (63, 65), (64, 64), (65, 63)]
BLOCKS = [(511, 513), (512, 512), (1023, 1025), (1024, 1024), (1025, 1023)]
STAGED = [(3072, 700), (3073, 700), (700, 3073)]
WIDE = [(64, 65536), (64, 65537), (65537, 64)]
CASES_A = ([case(n, m, hi=PLANT + 15 + 3 * i) for i, (n, m) in enumerate(SMALL)] +             # 25 .. 40 rotations
           [case(n, m, hi=PLANT + 30) for n, m in BLOCKS] +                                     # 40: batches of 32 and 8
           [case(n, m, hi=PLANT + 30) for n, m in STAGED] +
           [case(n, m, lo=PLANT - 1, hi=PLANT + 1) for n, m in WIDE] +
           [case(63, 65, lo=PLANT, hi=PLANT + 1)] +
           [case(63, 65, lo=PLANT - 10, hi=PLANT - 10 + k) for k in (31, 32, 33)] +            # the first-batch edge
           [case(63, 65, lo=PLANT - 100, hi=PLANT - 100 + k, batch_size=300, first_batch=300) for k in (256, 257)] +
           [case(63, 65, hi=PLANT + 30, batch_size=7)] +                                        # 7 does not divide 40 or 33
           [case(n, m, kind, hi=PLANT + 30) for n, m in ((1025, 1023), (3073, 700)) for kind in KINDS[1:]] +
           # At 1025 and 3073 points the last query block holds ONE query, so a later batch's rotation survives only if it beats
           # the best outright.  With a full last block the partial sums of an unalignable pair stay below the best: nothing
           # dies at either kill, the regime in which the merged second launch scans everything.
           [case(n, m, "unalignable", hi=PLANT + 30) for n, m in ((1536, 1400), (3584, 700))])


@functools.lru_cache(maxsize=None)
def oracle_of(n, m, kind):
    pred, gt = clouds(n, m, kind)
    return Oracle(pred, gt, sphere())


@functools.lru_cache(maxsize=None)
def oracle_record(c):
    n, m, kind, lo, hi, kw = c
    o = oracle_of(n, m, kind)
    mark = len(o.trace)
    rec = o.search(lo, hi, prune=False, **dict(kw))
    return rec, tuple(o.trace[mark:])


def last_tile_matters(c):
    """Per rotation of a WIDE case: is the long cloud's last sorted point - alone in candidate tile 64 - some query's nearest
    neighbour?  (The scan's own arithmetic, through the C oracle.)"""
    n, m, kind, lo, hi, _ = c
    o = oracle_of(n, m, kind)
    a = o.applied(np.arange(lo, hi), o.pred_s)
    _, _, i1, i2 = C.chamfer_forward(a, np.broadcast_to(o.gt_s, (hi - lo,) + o.gt_s.shape))
    return [bool((i == max(n, m) - 1).any()) for i in (i1 if m > n else i2)]


# section D
BOUND_PAIRS = ([("aligned", 300, 280, off, 1.0) for off in (0, 10, 100, 1000)] +
               [("aligned", 300, 280, 0, 1e-3), ("aligned", 300, 280, 0, 1e3), ("aligned", 5, 3, 0, 1.0), ("aligned", 1, 7, 0, 1.0),
                ("flat", 300, 280, 0, 1.0)])
BOUND_ROTATIONS = sorted(set(range(0, 6912, 7)) | set(range(PLANT - 3, PLANT + 4)))


@functools.lru_cache(maxsize=None)
def bound_clouds(kind, n, m, offset, scale):
    pred, gt = clouds(n, m, kind, seed=1)
    ext = float(np.ptp(pred, axis=0).max()) if n > 1 else 1.0
    pred = (pred.astype(F64) + offset * ext * np.array([1.0, -1.0, 0.5])) * scale
    gt = (gt.astype(F64) + offset * ext * np.array([-1.0, 0.5, 1.0])) * scale
    return np.ascontiguousarray(pred, F32), np.ascontiguousarray(gt, F32)


# =====================================================================================================
# GPU side
# =====================================================================================================
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_search(pred, gt, lo, hi, **kw):
    """brute_force_search -> (the record's first 12 words, best_pred, gt_n)."""
    from zeroshape_amd.utils import eval_3D as E
    out = E.brute_force_search(_cuda(pred), _cuda(gt), device="cuda", rotations=_cuda(sphere()), rot_slice=(lo, hi),
                               return_index=True, **kw)
    acc, comp, f, best_pred, gt_n, idx, cd = out
    rec = np.zeros(12, F32)
    rec[0], rec[2], rec[3], rec[4:10] = F32(cd), acc.item(), comp.item(), f.cpu().numpy()
    rec.view(np.int32)[1], rec.view(np.int32)[10], rec.view(np.int32)[11] = idx, E.brute_force_search.last_evaluated, E.brute_force_search.last_scanned
    return rec, best_pred.cpu().numpy(), gt_n[0].cpu().numpy()


def describe(rec):
    i = rec.view(np.int32)
    return "cd %.9g index %d acc %.9g comp %.9g f %s evaluated %d scanned %d" % (rec[0], i[1], rec[2], rec[3], rec[4:10], i[10], i[11])


@pytest.mark.parametrize("c", CASES_A, ids=case_id)
def test_record_is_bit_equal_to_the_oracle(c):
    n, m, kind, lo, hi, kw = c
    pred, gt = clouds(n, m, kind)
    want, trace = oracle_record(c)
    o = oracle_of(n, m, kind)
    print("A %s oracle: %s; batches (count, killed at stage 1, merged, dead): %s" % (case_id(c), describe(want), list(trace)))
    for nn in NN:
        got, best_pred, gt_n = gpu_search(pred, gt, lo, hi, prune=False, nn=nn, **dict(kw))
        print("  %s: %s" % (nn, describe(got)))
        same_bits(got.view(np.uint32), want[:12].view(np.uint32), "A %s nn=%s record (%s | %s)" % (case_id(c), nn, describe(got), describe(want)))
        same_bits(gt_n, o.gt_n, "A %s normalised ground truth" % case_id(c))
        same_bits(best_pred, o.applied(int(want.view(np.int32)[1]))[0], "A %s nn=%s best_pred" % (case_id(c), nn))


# ---- B. host-loop variants --------------------------------------------------------------------------
B_SIZE, B_SLICE = (1025, 1023), (PLANT - 300, PLANT + 300)


def gpu_bounds(pred, gt_n, lo, hi):
    from zeroshape_amd.utils import eval_3D as E
    return E._bf_lower_bounds(_cuda(pred), _cuda(gt_n), _cuda(sphere()[lo:hi])).cpu().numpy()


@pytest.mark.parametrize("peek", [True, False])
def test_pruned_search_with_and_without_peek_equals_the_oracle_fed_with_the_gpu_bounds(peek):
    o = oracle_of(B_SIZE[0], B_SIZE[1], "aligned")
    pred, gt = clouds(B_SIZE[0], B_SIZE[1], "aligned")
    lb = gpu_bounds(pred, o.gt_n, *B_SLICE)
    want = o.search(B_SLICE[0], B_SLICE[1], prune=True, peek=peek, lb=lb)
    other = o.search(B_SLICE[0], B_SLICE[1], prune=True, peek=not peek, lb=lb)
    same_bits(want.view(np.uint32), other.view(np.uint32), "B oracle: peek changes nothing")
    assert want.view(np.int32)[10] < B_SLICE[1] - B_SLICE[0], "the bounds must prune a batch, or peek is not exercised"
    for nn in NN:
        got, _, _ = gpu_search(pred, gt, B_SLICE[0], B_SLICE[1], prune=True, peek=peek, nn=nn)
        print("B peek=%s %s: %s" % (peek, nn, describe(got)))
        same_bits(got.view(np.uint32), want[:12].view(np.uint32), "B prune peek=%s nn=%s (%s | %s)" % (peek, nn, describe(got), describe(want)))


@pytest.mark.parametrize("first_batch", [1, 32, 256])
def test_first_batch_moves_the_counters_and_nothing_else(first_batch):
    o = oracle_of(B_SIZE[0], B_SIZE[1], "aligned")
    pred, gt = clouds(B_SIZE[0], B_SIZE[1], "aligned")
    want = o.search(B_SLICE[0], B_SLICE[1], prune=False, first_batch=first_batch)
    base = o.search(B_SLICE[0], B_SLICE[1], prune=False)
    same_bits(want[:10].view(np.uint32), base[:10].view(np.uint32), "B oracle: first_batch keeps cd, index and metrics")
    got, _, _ = gpu_search(pred, gt, B_SLICE[0], B_SLICE[1], prune=False, first_batch=first_batch)
    print("B first_batch=%d: %s" % (first_batch, describe(got)))
    same_bits(got.view(np.uint32), want[:12].view(np.uint32), "B first_batch=%d (%s | %s)" % (first_batch, describe(got), describe(want)))


class Abi(object):
    """zs_pose_search_batch_sorted called directly, on the clouds of an Oracle; the scratch is the test's to read."""

    def __init__(self, o, count, rotations):
        from zeroshape_amd import _lib
        from zeroshape_amd.utils import eval_3D as E
        self._lib, self.lib, self.o, self.count = _lib, _lib.load(), o, count
        self.pred, self.R = _cuda(o.pred), _cuda(rotations)
        self.pred_s, self.gt_s = E._spatially_sorted(self.pred), E._spatially_sorted(_cuda(o.gt_n))
        same_bits(self.pred_s.cpu().numpy(), o.pred_s, "sorted prediction")
        same_bits(self.gt_s.cpu().numpy(), o.gt_s, "sorted ground truth")
        self.thr = _cuda(o.thr)
        self.best = torch.empty(self.lib.zs_pose_best_bytes() // 4, dtype=torch.float32, device="cuda")
        self.gt_pack = torch.empty(self.lib.zs_pose_pack_bytes(o.m) // 4, dtype=torch.float32, device="cuda")
        self.scratch = torch.zeros(self.lib.zs_pose_sorted_scratch_bytes(o.n, o.m, count) // 4, dtype=torch.float32, device="cuda")
        self.st = _lib.current_stream_ptr(self.pred.device)
        _lib.check(self.lib.zs_pose_pack(_lib.ptr(self.gt_s), o.m, _lib.ptr(self.gt_pack), self.st), "zs_pose_pack")
        self.init()

    def init(self, bound=None):
        self._lib.check(self.lib.zs_pose_best_init(self._lib.ptr(self.best), self.st), "zs_pose_best_init")
        if bound is not None:
            self.best[12] = float(bound)

    def call(self, order, offset, mode=2, count=None, n=None, m=None, gt_pack=True, lb=None):
        o, p = self.o, self._lib.ptr
        self.order = None if order is None else _cuda(np.asarray(order, np.int32))
        count = (len(order) if order is not None else self.count) if count is None else count
        return self.lib.zs_pose_search_batch_sorted(p(self.pred), p(self.pred_s), o.n if n is None else n, p(self.gt_s),
                                                    p(self.gt_pack) if gt_pack else None, o.m if m is None else m, p(self.R),
                                                    None if order is None else p(self.order), count, offset, lb, p(self.thr),
                                                    p(self.best), p(self.scratch), mode, self.st)

    def record(self):
        return self.best.cpu().numpy()

    def flags(self, count):
        """(dead [count] bool, merge flag) of the last batch, from the scratch."""
        at = count * STAT + count * 2 * self.o.bx * PART
        d = self.scratch[at:at + DEAD_INTS].view(torch.int32).cpu().numpy()
        return d[:count] != 0, int(d[MERGE_SLOT])


def _abi_case(n=1025, m=1023):
    o = oracle_of(n, m, "aligned")
    local = sphere()[PLANT - 8:PLANT + 8].reshape(-1, 9).copy()        # 16 rotations; the planted one is local index 8
    lo = Oracle.__new__(Oracle)
    lo.__dict__.update(o.__dict__)
    lo.R, lo.part, lo.trace = local, {}, []
    return lo, local


def test_abi_duplicate_rotation_lowest_index_wins_and_index_offset_only_moves_the_index():
    o, local = _abi_case()
    R = np.concatenate([local, local[8:9]])                              # index 16 repeats the planted rotation
    o.R = R
    abi = Abi(o, 8, R)
    for order in ([16, 3, 8, 5], [8, 3, 16, 5], [5, 16, 3]):
        abi.init()
        assert abi.call(order, 0) == 1
        want = new_record()
        o.batch(want, np.array(order), np.array(order))
        same_bits(abi.record().view(np.uint32), want.view(np.uint32), "B duplicate order %s" % order)
        assert int(want.view(np.int32)[1]) == min(k for k in order if k in (8, 16))
    # the same batch twice: offset 100, then offset 0 - the tie on cd goes to the lower index, nothing else moves
    order = [2, 8, 11, 4]
    abi.init()
    assert abi.call(order, 100) == 1
    first = abi.record().copy()
    assert abi.call(order, 0) == 1
    second = abi.record()
    want = new_record()
    o.batch(want, np.array(order), np.array(order) + 100)
    same_bits(first.view(np.uint32), want.view(np.uint32), "B offset 100")
    o.batch(want, np.array(order), np.array(order))
    same_bits(second.view(np.uint32), want.view(np.uint32), "B offset 100 then 0")
    assert first.view(np.int32)[1] == 108 and second.view(np.int32)[1] == 8
    same_bits(second[[0, 2, 3, 4, 5, 6, 7, 8, 9]], first[[0, 2, 3, 4, 5, 6, 7, 8, 9]], "B offset: cd and metrics unchanged")
    # ... and the other way round the higher index does not replace the lower one
    assert abi.call(order, 100) == 1
    assert abi.record().view(np.int32)[1] == 8


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_abi_external_bound_dead_flags_and_merge_flag(mode):
    o, local = _abi_case()
    assert o.bx >= 3
    abi = Abi(o, 16, local)
    order = np.arange(16)
    cds = np.sort(o.cd_of(order))
    stat = np.sort(o.kill_stat(o.partials(order), STAGE_ENDS[0]))
    assert cds[0] < cds[1] and len(set(stat.tolist())) == 16

    def run(bound, idx, what):
        abi.init(bound)
        abi.scratch.fill_(float("nan"))
        assert abi.call(idx, 0, mode=mode) == 1
        want = new_record(bound)
        dead = o.batch(want, np.array(idx), np.array(idx))
        got_dead, got_merge = abi.flags(len(idx))
        print("B bound %s (%s): oracle dead %d merged %s | gpu dead %d merged %d" % (bound, what, dead.sum(), o.merged, got_dead.sum(), got_merge))
        same_bits(abi.record().view(np.uint32), want.view(np.uint32), "B %s record" % what)
        assert np.array_equal(got_dead, dead), (what, got_dead, dead)
        assert got_merge == int(o.merged), (what, got_merge, o.merged)
        return want, dead

    free, dead = run(np.inf, order, "no bound")
    assert not dead.any() and o.merged
    # below every cd: all die, and the record is the all-dead one: (+inf, lowest index, zeros), scanned 0
    want, dead = run(F32(stat[0]) / F32(2), order, "bound below every cd")
    assert dead.all() and not o.merged
    assert np.isinf(want[0]) and want.view(np.int32)[1] == 0 and not want[2:10].any() and want.view(np.int32)[11] == 0
    # between the best and the second-best cd: the winner's record, as without a bound
    mid = F32((F64(cds[0]) + F64(cds[1])) / 2)
    assert cds[0] < mid < cds[1]
    want, dead = run(mid, order, "bound between best and second")
    same_bits(want[:10].view(np.uint32), free[:10].view(np.uint32), "B bound between: record unchanged")
    # the merge decision on both sides of 4 * killed == count: 3, 4 and 5 of 16 killed at the first stage
    for killed in (3, 4, 5):
        b = F32((F64(stat[15 - killed]) + F64(stat[16 - killed])) / 2)
        assert stat[15 - killed] < b < stat[16 - killed]
        want, dead = run(b, order, "%d of 16 killed at stage 1" % killed)
        assert o.trace[-1][1] == killed and o.merged == (killed <= 4)
    # ... and of 8: 2 killed merges, 3 does not
    sub = np.argsort(o.kill_stat(o.partials(order), STAGE_ENDS[0]), kind="stable")[-8:]
    s8 = np.sort(o.kill_stat(o.partials(sub), STAGE_ENDS[0]))
    for killed in (2, 3):
        b = F32((F64(s8[7 - killed]) + F64(s8[8 - killed])) / 2)
        want, dead = run(b, list(sub), "%d of 8 killed at stage 1" % killed)
        assert o.trace[-1][1] == killed and o.merged == (killed <= 2)


def test_abi_refusals_come_before_any_launch():
    o, local = _abi_case(63, 65)
    big = np.tile(local, (17, 1))[:257]
    abi = Abi(o, 256, big)
    abi.init(0.125)
    torch.cuda.synchronize()
    before = abi.record().copy()
    err = lambda: abi.lib.zs_last_error().decode()
    assert abi.call(None, 0, count=257) == 0 and err() == "zs_pose_search_batch_sorted: 257 rotations per batch exceed 256"
    assert abi.call(None, 0, count=4, n=0) == 0 and err() == "zs_pose_search_batch_sorted: empty cloud (n=0 m=65)"
    assert abi.call(None, 0, count=4, m=0) == 0 and err() == "zs_pose_search_batch_sorted: empty cloud (n=63 m=0)"
    assert abi.call(None, 0, count=4, n=-1) == 0 and err() == "zs_pose_search_batch_sorted: negative size (n=-1 m=65 count=4)"
    assert abi.call(None, 0, count=-4) == 0 and err() == "zs_pose_search_batch_sorted: negative size (n=63 m=65 count=-4)"
    assert abi.call(None, 0, count=4, gt_pack=False) == 0 and err() == "zs_pose_search_batch_sorted: null pointer or bad mode"
    assert abi.call(None, 0, count=4, mode=3) == 0 and err() == "zs_pose_search_batch_sorted: null pointer or bad mode"
    assert abi.call(None, 0, count=0) == 1
    torch.cuda.synchronize()
    same_bits(abi.record().view(np.uint32), before.view(np.uint32), "B refusals leave the record alone")
    # (mode 0 does not need the pack: the same null pointer is accepted there)
    abi.init()
    assert abi.call(None, 0, count=4, gt_pack=False, mode=0) == 1
    want = new_record()
    o.R = big
    o.batch(want, np.arange(4), np.arange(4))
    same_bits(abi.record().view(np.uint32), want.view(np.uint32), "B mode 0 without a pack")


# ---- C. zs_pose_pack and zs_str_sort alone ----------------------------------------------------------
PACK_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
SORT_SIZES = [1, 2, 63, 64, 65, 128, 129, 4096, 4097, 10000]
SENTINEL = -12345.0


@functools.lru_cache(maxsize=None)
def pack_cloud(n, non_finite):
    p = _rs(8, n).uniform(-1, 1, (n, 3)).astype(F32)
    if non_finite:                                           # three sub-tiles (n = 2049: also three tiles), three coordinates
        p[n // 7, 0], p[n // 2, 1], p[n - 1, 2] = np.nan, np.inf, -np.inf
        if n >= 130:
            p[64:128] = np.nan                               # a sub-tile without one finite coordinate: the empty box
    return p


@pytest.mark.parametrize("n,non_finite", [(n, False) for n in PACK_SIZES] + [(n, True) for n in (65, 1025, 2049)])
def test_pack_is_bit_equal_to_numpy(n, non_finite):
    from zeroshape_amd import _lib
    lib = _lib.load()
    p = pack_cloud(n, non_finite)
    want = pack_ref(p)
    assert lib.zs_pose_pack_bytes(n) == want.size * 4
    pts = _cuda(p)
    buf = torch.full((want.size + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    _lib.check(lib.zs_pose_pack(_lib.ptr(pts), n, _lib.ptr(buf), _lib.current_stream_ptr(pts.device)), "zs_pose_pack")
    got = buf.cpu().numpy()
    same_bits(got[:want.size], want, "C pack n=%d" % n)
    assert (got[want.size:] == F32(SENTINEL)).all(), "C pack n=%d writes behind zs_pose_pack_bytes" % n


@functools.lru_cache(maxsize=None)
def sort_cloud(n):
    p = _rs(9, n).uniform(-1, 1, (n, 3)).astype(F32)
    if n >= 63:
        p[0:8, 0] = 0.25                                     # equal x, different y
        p[8] = p[9] = p[40]                                  # exact duplicates
        p[10, 0], p[11, 0], p[12, 1], p[13, 1], p[14, 2], p[15, 2] = 0.0, -0.0, -0.0, 0.0, 0.0, -0.0
        p[16, 0], p[17, 0], p[18, 1], p[19, 2] = 1e-40, -1e-40, 3e-45, -3e-45          # denormals
        p[20, 0], p[30, 1], p[n // 2, 2] = np.nan, np.inf, -np.inf
    elif n == 2:
        p[0, 0], p[1, 0] = 0.0, -0.0
    return p


@pytest.mark.parametrize("n", SORT_SIZES)
def test_str_sort_is_bit_equal_to_the_restated_order(n):
    from zeroshape_amd import _lib
    lib = _lib.load()
    p = sort_cloud(n)
    want = str_order(p)
    pts = _cuda(p)
    st = _lib.current_stream_ptr(pts.device)
    scratch = torch.empty(lib.zs_str_scratch_bytes(n) // 4 + 1, device="cuda")
    out, perm = torch.full_like(pts, SENTINEL), torch.full((n,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.zs_str_sort(_lib.ptr(pts), n, _lib.ptr(out), _lib.ptr(perm), _lib.ptr(scratch), st), "zs_str_sort")
    same_bits(perm.cpu().numpy(), want, "C sort n=%d perm" % n)
    same_bits(out.cpu().numpy(), p[want], "C sort n=%d sorted" % n)
    out2 = torch.full_like(pts, SENTINEL)
    _lib.check(lib.zs_str_sort(_lib.ptr(pts), n, _lib.ptr(out2), None, _lib.ptr(scratch), st), "zs_str_sort")
    same_bits(out2.cpu().numpy(), p[want], "C sort n=%d sorted, perm=None" % n)


# ---- D. the lower bounds ----------------------------------------------------------------------------
@pytest.mark.parametrize("pair", BOUND_PAIRS, ids=lambda p: "%s-%dx%d-off%g-x%g" % p)
def test_lower_bounds_stay_below_the_exact_distance(pair):
    pred, gt = bound_clouds(*pair)
    o = Oracle(pred, gt, sphere())
    rot = np.array(BOUND_ROTATIONS)
    from zeroshape_amd.utils import eval_3D as E
    lb = E._bf_lower_bounds(_cuda(pred), _cuda(o.gt_n), _cuda(sphere()[rot])).cpu().numpy()
    cd = o.cd_of(rot)
    slack = cd.astype(F64) - (lb.astype(F64) * (1 - 1e-3) - 1e-6)
    worst = int(np.argmin(slack))
    print("D %s: %d rotations, lb in [%.6g, %.6g], cd in [%.6g, %.6g], smallest cd - (lb (1 - 1e-3) - 1e-6) = %.6g at rotation %d"
          % (pair, len(rot), lb.min(), lb.max(), cd.min(), cd.max(), slack[worst], rot[worst]))
    assert np.isfinite(lb).all() and (lb >= 0).all()
    assert (slack >= 0).all(), "%d bounds exceed the exact distance" % int((slack < 0).sum())


def test_pruning_an_off_centre_pair_over_the_whole_sphere_changes_nothing():
    from zeroshape_amd.utils import eval_3D as E
    pred, gt = bound_clouds("aligned", 300, 280, 1000, 1.0)
    full, bp_full, _ = gpu_search(pred, gt, 0, 6912, prune=False)
    fast, bp_fast, _ = gpu_search(pred, gt, 0, 6912, prune=True)
    print("D end to end: exhaustive %s | pruned %s" % (describe(full), describe(fast)))
    same_bits(fast[:10].view(np.uint32), full[:10].view(np.uint32), "D pruned record")
    same_bits(bp_fast, bp_full, "D pruned best_pred")
    assert fast.view(np.int32)[10] < full.view(np.int32)[10] == 6912
