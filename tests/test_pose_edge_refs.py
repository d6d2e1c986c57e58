"""CPU side of tests/test_gpu_pose_edges.py: the evidence that its oracle, its cases and its constants are sound.

 - constants and launcher conditions: read from the source text and required verbatim, so a launcher that changes shape
   fails here instead of being restated wrongly;
 - branch accounting: a restatement of search_batch's stage loop, pack_subs and T maps every case of sections A to C to the
   branches it takes; every named branch must have a case on each side of its threshold (T of 64 and 65, bx of 2 / 3 and
   6 / 7, merged and unmerged stages, a first batch of 32 / 33, the batch clamp);
 - the oracle is sound: on the section A cases up to 1025 points its winner equals that of oracle.geometry_ref's
   brute_force_search (the restatement of the reference itself), acc / comp / cd agree within the "measured" rule -
   max(1e-5 relative: the tolerance of test_brute_force_search_matches_oracle_scan; 4 x the error of the fp32 reference
   restatement against a float64 one on the same input) - and the F-scores are equal;
 - the restatements are sound: the STR order is a permutation with the non-finite points last, the pack boxes contain their
   points, and the predicted kill counts show both merge regimes."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import geometry_ref as G
from tests import test_gpu_pose_edges as P
from tests.test_eval_edge_refs import _int, _source, launcher

F32, F64 = np.float32, np.float64
REL_TOL_EXISTING = 1e-5            # tests/test_gpu_chamfer.py::test_brute_force_search_matches_oracle_scan


# =====================================================================================================
# constants and conditions, verbatim
# =====================================================================================================
class Constants(object):
    def __init__(self):
        pose, sort = _source("zeroshape_amd", "csrc", "pose_search.hip"), _source("zeroshape_amd", "csrc", "morton_sort.hip")
        prune, host = _source("zeroshape_amd", "csrc", "bf_prune.hip"), _source("zeroshape_amd", "utils", "eval_3D.py")
        self.threads = _int(r"constexpr int PS_THREADS = (\d+);", pose)
        self.q = _int(r"constexpr int PS_Q = (\d+);", pose)
        self.tile = _int(r"constexpr int PS_TILE = (\d+);", pose)
        self.sub = _int(r"constexpr int PS_SUB = (\d+);", pose)
        self.part = _int(r"constexpr int PS_PART = (\d+);", pose)
        self.stat = _int(r"constexpr int PS_STAT = (\d+);", pose)
        self.leaf = _int(r"constexpr int STR_LEAF = (\d+);", sort)
        self.lb_axis = _int(r"constexpr int LB_AXIS = (\d+);", prune)
        self.dead_extra = _int(r"constexpr int PS_DEAD_INTS = PS_THREADS \+ (\d+);", pose)
        a, b, c = re.findall(r"int stage_end\[4\] = \{(\d+), (\d+), (\d+), bx\};", pose)[0]
        self.stage_end = (int(a), int(b), int(c))
        flat = re.sub(r"\s+", " ", pose)
        for line in (
                "constexpr int PS_MERGE_SLOT = PS_THREADS;",
                "constexpr int PS_NSUB = PS_TILE / PS_SUB;",
                "return lower_bound && lower_bound[0] * (1.0f - 1e-3f) - 1e-6f > prune_bound(best);",
                "__device__ __forceinline__ float prune_bound(const float *best) { return fminf(best[0], best[12]); }",
                "if (!CULL || T > 64) {",
                "const int T = ncs / PS_NSUB;",
                "if (lane < T) {",
                "j = j < nq ? j : nq - 1;",
                "if (decide_merge && threadIdx.x == 0) dead[PS_MERGE_SLOT] = 4 * killed <= count ? 1 : 0;",
                "return (s[0] / (float)n + s[1] / (float)m) / 2.f > bst;",
                "if (win_cd < old_cd || (win_cd == old_cd && win_idx < old_idx)) {",
                "if (c2 < s_cd[tid] || (c2 == s_cd[tid] && i2 < s_idx[tid])) {",
                "ibest[10] += count;", "ibest[11] += s_alive;",
                "if (cd != cd) cd = INFINITY;",
                "__host__ __device__ inline int pack_subs(int n) { return (n + PS_TILE - 1) / PS_TILE * PS_NSUB; }",
                "return mode == 1 ? (bx >= end && !merged) : merged;",
                # search_batch's stage loop, as stage_plan() below restates it
                "for (int sidx = 0; sidx < 4 && lo < bx; sidx++) {",
                "const int hi = stage_end[sidx] < bx ? stage_end[sidx] : bx;",
                "if (hi <= lo) continue;",
                "const int smode = launched == 0 ? 0 : launched == 1 ? 1 : 2;",
                "const int span = smode == 1 ? bx - lo : hi - lo;",
                "if (hi < bx) hipLaunchKernelGGL(pose_kill_kernel,",
                "lower_bound, launched == 0 ? 1 : 0);",
                "if (count > PS_THREADS) {",
                'extern "C" int zs_pose_max_batch(void) { return PS_THREADS; }',
                "const float s = sqrtf(bestd[q]);",
                "const float lx = (xmax - mx) - (xmin - mx), ly = (ymax - my) - (ymin - my);",
                "s[12] = fmaxf(lx, ly) + 1.e-7f;"):
            assert line in flat, "pose_search.hip no longer reads: %s" % line
        flat = re.sub(r"\s+", " ", sort)
        for line in ("const int leaves = ceil_div(n, STR_LEAF), slabs = ceil_cbrt(leaves);",
                     "return StrPlan{n, per * STR_LEAF, ceil_sqrt(per)};",
                     "const int begin = slab * pl.slab_points, len = min(pl.slab_points, pl.n - begin);",
                     "const int leaves = ceil_div(len, STR_LEAF), strips = ceil_sqrt(leaves), per = ceil_div(leaves, strips);",
                     "return slab * pl.max_strips + (i - begin) / (per * STR_LEAF);",
                     "const unsigned lo = ok ? ordered_bits(v) : 0xffffffffu;",
                     "return (u & 0x80000000u) ? ~u : (u | 0x80000000u);"):
            assert line in flat, "morton_sort.hip no longer reads: %s" % line
        for line in ("batch_size = min(int(batch_size), lib.zs_pose_max_batch())",
                     "first_batch = min(batch_size, 32) if first_batch is None else max(1, min(int(first_batch), batch_size))",
                     "if prune and (K > batch_size or rot_shard is not None):",
                     "lb_sorted, order = torch.sort(lb, stable=True)",
                     "if peek and lb_sorted is not None and bi in (2, 4) and not torch.cuda.is_current_stream_capturing():",
                     "if np.float32(np.float32(lb_host[pos]) * np.float32(1.0 - 1e-3)) - np.float32(1e-6) > bound:"):
            assert line in host, "eval_3D.py no longer reads: %s" % line
        text = launcher(pose, "zs_pose_pack")
        assert "dim3(pack_subs(points) / PS_NSUB, 1), dim3(PS_TILE)" in text


@pytest.fixture(scope="module")
def K():
    return Constants()


def test_the_gpu_module_restates_the_constants_of_the_source(K):
    assert (P.THREADS, P.Q_PER_LANE, P.TILE, P.SUB, P.LEAF) == (K.threads, K.q, K.tile, K.sub, K.leaf)
    assert (P.MAX_BATCH, P.MERGE_SLOT, P.DEAD_INTS, P.STAT, P.PART) == (K.threads, K.threads, K.threads + K.dead_extra, K.stat, K.part)
    assert K.stage_end == (P.STAGE_ENDS[0], P.STAGE_ENDS[1], P.STAGE_ENDS[1]) and K.lb_axis == 32
    # 1.0f - 1e-3f (fp32 constants folded in fp32) and the host loop's float32(1.0 - 1e-3) are one number
    assert F32(1.0) - F32(1e-3) == F32(1.0 - 1e-3)


# =====================================================================================================
# branch accounting
# =====================================================================================================
def stage_plan(K, bx):
    """search_batch's loop: [(mode, first block, end of own range, blocks spanned, kill behind it, that kill decides the merge)]."""
    out, lo, launched = [], 0, 0
    for end in K.stage_end + (bx,):
        if lo >= bx:
            break
        hi = min(end, bx)
        if hi <= lo:
            continue
        mode = min(launched, 2)
        out.append((mode, lo, hi, bx - lo if mode == 1 else hi - lo, hi < bx, launched == 0))
        lo, launched = hi, launched + 1
    return out


def tiles(K, points):
    return P.ceil_div(points, K.tile)


def search_branches(K, c, trace):
    n, m, kind, lo, hi, kw = c
    kw = dict(kw)
    bx = P.ceil_div(max(n, m), K.threads * K.q)
    names = {"bx=%d" % bx if bx in (1, 2, 3, 6, 7) else "bx>7" if bx > 7 else "bx 4..5"}
    plan = stage_plan(K, bx)
    names.add("%d launches, %d kills" % (len(plan), sum(p[4] for p in plan)))
    for d, (q, cand) in enumerate(((n, m), (m, n))):
        T = tiles(K, cand)
        names.add("T=64" if T == 64 else "T=65: all-pairs fallback" if T == 65 else "T<64" if T < 64 else "T>65")
        names.add("queries: %s" % ("one" if q == 1 else "below a sub-tile" if q < K.sub else "a sub-tile" if q == K.sub else
                                   "ragged block" if q % (K.threads * K.q) else "whole blocks"))
        if q % (K.threads * K.q) and q % (K.threads * K.q) <= K.threads:
            names.add("slot 1 of the last block all clamped")
    Kr, bs = hi - lo, min(kw.get("batch_size", 256), K.threads)
    if kw.get("batch_size", 256) > K.threads:
        names.add("batch clamp, %d rotations" % Kr)
    first = min(bs, 32) if "first_batch" not in kw else max(1, min(kw["first_batch"], bs))
    names.add("first batch: %s" % ("slice below it" if Kr < first else "slice equals it" if Kr == first else
                                   "one rotation behind it" if Kr == first + 1 else "more behind it"))
    if (Kr - first) % bs and Kr > first + 1:
        names.add("ragged last batch")
    for count, killed1, merged, dead in trace:
        if merged is not None:
            fresh = "first batch" if (count, killed1, merged, dead) == trace[0] else "later batch"
            names.add("%s: %s%s" % (fresh, "merged" if merged else "unmerged",
                                    "" if fresh == "first batch" else ", none dead" if dead == 0 else ", all dead" if dead == count else ", some dead"))
    return names


def test_section_a_cases_sit_on_both_sides_of_every_threshold(K):
    assert stage_plan(K, 1) == [(0, 0, 1, 1, False, True)]
    assert stage_plan(K, 2) == [(0, 0, 2, 2, False, True)]
    assert stage_plan(K, 3) == [(0, 0, 2, 2, True, True), (1, 2, 3, 1, False, False)]
    assert stage_plan(K, 6) == [(0, 0, 2, 2, True, True), (1, 2, 6, 4, False, False)]
    assert stage_plan(K, 7) == [(0, 0, 2, 2, True, True), (1, 2, 6, 5, True, False), (2, 6, 7, 1, False, False)]
    seen = {}
    for c in P.CASES_A:
        _, trace = P.oracle_record(c)
        for name in search_branches(K, c, trace):
            seen.setdefault(name, []).append(P.case_id(c))
    for name in sorted(seen):
        print("%-45s %d cases, e.g. %s" % (name, len(seen[name]), seen[name][0]))
    need = ["bx=1", "bx=2", "bx=3", "bx=6", "bx=7", "bx>7", "1 launches, 0 kills", "2 launches, 1 kills", "3 launches, 2 kills",
            "T<64", "T=64", "T=65: all-pairs fallback",
            "queries: one", "queries: below a sub-tile", "queries: a sub-tile", "queries: ragged block", "queries: whole blocks",
            "slot 1 of the last block all clamped",
            "batch clamp, 256 rotations", "batch clamp, 257 rotations",
            "first batch: slice below it", "first batch: slice equals it", "first batch: one rotation behind it",
            "first batch: more behind it", "ragged last batch",
            "first batch: merged", "later batch: unmerged, all dead", "later batch: merged, none dead", "later batch: merged, some dead"]
    missing = [name for name in need if name not in seen]
    assert not missing, missing
    # T == 65 is reached with the long cloud as candidates of direction 0 and of direction 1
    wide = [c for c in P.CASES_A if max(c[0], c[1]) > 65536]
    assert {c[0] > c[1] for c in wide} == {True, False} and all(c[4] - c[3] == 2 and min(c[0], c[1]) == 64 for c in wide)
    for c in wide:
        if max(c[0], c[1]) == 65537:
            long_cloud = P.clouds(*c[:3])[0] if c[0] > c[1] else P.oracle_of(*c[:3]).gt_n
            assert P.str_order(long_cloud)[-1] == 0 and all(P.last_tile_matters(c)), "tile 64 must hold some query's nearest neighbour"
    # the largest oracle call
    assert max(c[0] * c[1] * (c[4] - c[3]) for c in P.CASES_A if max(c[0], c[1]) < 65536) <= 3584 * 700 * 40


def test_kill_counts_show_both_merge_regimes():
    """More than a quarter of the later batch killed at the first stage on the aligned pairs (unmerged), none on the
    unalignable ones whose last query block is full (merged, and nothing dies at the later kill either)."""
    for n, m in ((1025, 1023), (3073, 700)):
        _, trace = P.oracle_record(P.case(n, m, "aligned", hi=P.PLANT + 30))
        count, killed1, merged, dead = trace[1]
        print("aligned %dx%d: batch of %d, %d killed at stage 1, merged %s, %d dead" % (n, m, count, killed1, merged, dead))
        assert 4 * killed1 > count and merged is False and trace[0][2] is True
    for n, m in ((1536, 1400), (3584, 700)):
        _, trace = P.oracle_record(P.case(n, m, "unalignable", hi=P.PLANT + 30))
        count, killed1, merged, dead = trace[1]
        print("unalignable %dx%d: batch of %d, %d killed at stage 1, merged %s, %d dead" % (n, m, count, killed1, merged, dead))
        assert killed1 == 0 and dead == 0 and merged is True
    # merged by the first kill, thinned by the second: the later kill kernels still act on a merged batch
    _, trace = P.oracle_record(P.case(3073, 700, "unalignable", hi=P.PLANT + 30))
    assert trace[1][1] == 0 and trace[1][2] is True and trace[1][3] == trace[1][0]


def test_sections_b_and_c_cover_their_edges(K):
    assert P.ceil_div(max(P.B_SIZE), K.threads * K.q) >= 3 and P.B_SLICE[1] - P.B_SLICE[0] == 600
    sub, tile = K.sub, K.tile
    assert {1, sub - 1, sub, sub + 1, tile - 1, tile, tile + 1, 2 * tile + 1} == set(P.PACK_SIZES)
    plans = {n: P.str_plan(n) for n in P.SORT_SIZES}
    assert plans[65] == (65, 64, 1) and plans[64] == (64, 64, 1)             # 65: two slabs of one leaf, the second ragged
    assert plans[129] == (129, 128, 2) and plans[4097][1] % K.leaf == 0
    assert any(n % plans[n][1] for n in P.SORT_SIZES) and any(n % plans[n][1] == 0 for n in P.SORT_SIZES)   # ragged last slab
    groups = P.str_group(plans[10000], np.arange(10000), 2)
    assert (np.diff(groups) >= 0).all() and len(set(groups.tolist())) > plans[10000][2]
    leaves_cut = np.flatnonzero(np.diff(groups)) + 1
    assert (leaves_cut % K.leaf == 0).all(), "strips are cut in whole leaves"


# =====================================================================================================
# the oracle is sound
# =====================================================================================================
SOUND = [c for c in P.CASES_A if max(c[0], c[1]) <= 1025 and not dict(c[5]) and c[4] - c[3] >= 24]


def f64_search(pred, gt, R):
    """The reference's search in float64 on the same float32 inputs -> per rotation (acc, comp, cd) and the two distance sets."""
    p, g = pred.astype(F64), gt.astype(F64)

    def norm(x):
        x = x - x.mean(0)
        return x / (max(np.ptp(x[:, 0]), np.ptp(x[:, 1])) + 1e-7)
    g = norm(g)
    out, dists = [], []
    for r in R.astype(F64):
        q = norm(p @ r.T)
        d = np.sqrt(((q[:, None, :] - g[None, :, :]) ** 2).sum(2))
        d1, d2 = d.min(1), d.min(0)
        out.append((d1.mean(), d2.mean(), (d1.mean() + d2.mean()) / 2))
        dists.append((d1, d2))
    return np.array(out), dists


def fp32_reference(pred, gt, R):
    """oracle.geometry_ref.brute_force_search (the reference's own ops in torch fp32), and per rotation (acc, comp, cd)."""
    Rt = torch.from_numpy(np.ascontiguousarray(R))
    best = G.brute_force_search(torch.from_numpy(pred), torch.from_numpy(gt), rotations=Rt)
    rows = []
    for k in range(len(R)):
        acc, comp, _, _, _, _ = G.brute_force_search(torch.from_numpy(pred), torch.from_numpy(gt), rotations=Rt[k:k + 1])
        rows.append((float(acc), float(comp), (float(acc) + float(comp)) / 2))
    return best, np.array(rows)


NOISE = {}


@pytest.mark.parametrize("c", SOUND, ids=P.case_id)
def test_oracle_agrees_with_the_reference_restatement(c):
    n, m, kind, lo, hi, _ = c
    pred, gt = P.clouds(n, m, kind)
    R = P.sphere()[lo:hi]
    want, _ = P.oracle_record(c)
    o = P.oracle_of(n, m, kind)
    best, ref32 = fp32_reference(pred, gt, R)
    ref64, dists = f64_search(pred, gt, R)
    # The noise is ABSOLUTE: a rounding moves a normalised point by ~1e-6 whatever the rotation, and a metric follows such a
    # move at first order (measured on the offset pair: a rigid shift of 4.2e-6 moves acc by 3.9e-7), so the error of a mean
    # distance does not shrink with the distance.  Per metric: the largest |fp32 reference - float64| over the slice.
    noise = np.abs(ref32 - ref64).max(0)
    widx = int(want.view(np.int32)[1])
    w64 = ref64[widx - lo]
    tol = np.maximum(REL_TOL_EXISTING * np.abs(w64), 4 * noise)
    NOISE[P.case_id(c)] = (noise, tol / np.maximum(np.abs(w64), 1e-30))
    print("%s: noise of the fp32 reference (acc, comp, cd) %s absolute, tolerance %s; winner %d" % (P.case_id(c), noise, tol, widx))
    assert widx == lo + int(best[5])
    for i, (name, got) in enumerate((("acc", want[2]), ("comp", want[3]), ("cd", want[0]))):
        print("  %s: oracle %.9g, float64 %.9g, off by %.3g" % (name, got, w64[i], abs(float(got) - w64[i])))
        assert abs(float(got) - w64[i]) <= tol[i], (name, got, w64[i], tol[i])
    # the seed: the runner-up is farther behind the winner than 8 x that noise (ties in every rotation: one-point clouds)
    cds = np.sort(ref64[:, 2])
    if cds[-1] > cds[0]:
        assert cds[1] - cds[0] > 8 * noise[2], (cds[:3], noise)
    else:
        assert n == 1
    # F-scores: equal to the reference's, and no distance of the winner within the noise of a threshold
    near = sum(int((np.abs(d - t) <= max(REL_TOL_EXISTING * t, 4 * noise[j])).sum()) for j, d in enumerate(dists[widx - lo])
               for t in P.THRESHOLDS)
    assert near == 0, "%d distances within the noise of a threshold: choose another seed" % near
    np.testing.assert_array_equal(want[4:10], best[2].numpy())
    # ... and the oracle's own per-rotation cd picks the same winner with the reference's rule (first strict minimum)
    cd = o.cd_of(np.arange(lo, hi))
    assert lo + int(np.argmin(cd)) == widx


def test_measured_noise_is_what_the_note_records():
    """profiles/pose_edge_checks.md quotes these.  The tolerance is 1e-5 relative (the existing test's) wherever 4 x noise
    stays below it; only the pair translated by 100 x its extent, where fp32 has lost seven bits before the first
    subtraction, may exceed it - and stays below 1e-2."""
    for c in SOUND:
        if P.case_id(c) not in NOISE:
            test_oracle_agrees_with_the_reference_restatement(c)
    for name in sorted(NOISE):
        print("%-40s noise %s, tolerance relative to the winner %s" % (name, NOISE[name][0], NOISE[name][1]))
    wide = sorted(name for name in NOISE if (NOISE[name][1][2] > 1.0001 * REL_TOL_EXISTING))
    print("cd tolerance above 1e-5 relative:", wide)
    assert all(NOISE[name][1].max() < 1e-2 for name in NOISE)


# =====================================================================================================
# the restatements are sound
# =====================================================================================================
@pytest.mark.parametrize("n", P.SORT_SIZES)
def test_str_restatement_is_a_permutation_with_the_non_finite_points_last(n):
    p = P.sort_cloud(n)
    perm = P.str_order(p)
    assert sorted(perm.tolist()) == list(range(n))
    bad = ~np.isfinite(p).all(1)
    k = int(bad.sum())
    assert k == (3 if n >= 63 else 0)
    if k:
        plan = P.str_plan(n)
        # they close the last slab's last strip ... (pass 0 sends them to the end, later passes keep them at their group's end)
        assert bad[perm[-1]] and set(np.flatnonzero(bad)) <= set(perm[-(min(n, plan[1])):].tolist())
    if n >= 63:
        s = p[perm]
        at = {tuple(np.flatnonzero((s.view(np.uint32) == p[i].view(np.uint32)).all(1))) for i in (8, 9, 40)}
        assert len(at) == 1 and len(next(iter(at))) == 3                       # the three duplicates end up adjacent
        dup = sorted(next(iter(at)))
        assert dup[2] - dup[0] == 2 and perm[dup].tolist() == [8, 9, 40]       # ... in input order: the sorts are stable
    assert P.ordered_bits(np.array([-0.0], F32))[0] < P.ordered_bits(np.array([0.0], F32))[0]
    v = np.array([-np.inf, -1.0, -1e-40, -0.0, 0.0, 3e-45, 1e-40, 1.0, np.inf], F32)
    assert (np.diff(P.ordered_bits(v).astype(np.int64)) > 0).all()


@pytest.mark.parametrize("n,non_finite", [(n, False) for n in P.PACK_SIZES] + [(n, True) for n in (65, 1025, 2049)])
def test_pack_restatement_boxes_contain_their_points(K, n, non_finite):
    p = P.pack_cloud(n, non_finite)
    buf = P.pack_ref(p)
    ns = P.ceil_div(n, K.tile) * (K.tile // K.sub)
    assert buf.size == ns * 3 * K.sub + ns * 8 + ns // 16 * 8
    coords = buf[:ns * 3 * K.sub].reshape(ns, 3, K.sub)
    box = buf[ns * 3 * K.sub:ns * 3 * K.sub + ns * 8].reshape(ns, 8)
    tbox = buf[ns * 3 * K.sub + ns * 8:].reshape(ns // 16, 8)
    assert not box[:, 6:].any() and not tbox[:, 6:].any()
    for s in range(ns):
        pts = p[s * K.sub:(s + 1) * K.sub]
        for a in range(3):
            fin = pts[:, a][np.isfinite(pts[:, a])]
            if len(fin):
                assert box[s, a] == fin.min() and box[s, 3 + a] == fin.max()
            else:
                assert box[s, a] == np.inf and box[s, 3 + a] == -np.inf
            assert box[s, a] >= tbox[s // 16, a] and box[s, 3 + a] <= tbox[s // 16, 3 + a]
        got = coords[s].T[:len(pts)]
        assert np.array_equal(got.view(np.uint32), pts.view(np.uint32)) and np.isposinf(coords[s].T[len(pts):]).all()
    if non_finite and n >= 130:
        assert np.isposinf(box[1, 0:3]).all() and np.isneginf(box[1, 3:6]).all()      # the all-NaN sub-tile: the empty box
