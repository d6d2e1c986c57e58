"""CPU side of tests/test_gpu_eval_edges.py: the evidence that its references, tolerances and cases are sound.

 - branch accounting: a restatement of the launcher conditions of zs_chamfer_forward, chamfer_3D.forward's method="auto",
   axis_cells(), zs_chamfer_backward, zs_normalize_pc, zs_icp_step and zs_depth_metrics, with every constant read from the
   source text, maps each case of the GPU module to the branches it takes; every named branch must have a case and the
   cases must sit on both sides of every threshold - all sixteen grid sizes, both instantiations of the brute scan and
   the five arms by which icp_fit_kernel forms a singular triplet's u_i;
 - references: the numpy restatement of the non-finite contract equals the C oracle on every finite / +inf case of
   sections A and B, in every batch element (all queries; in the two largest cases of A and the cases of B above 360
   points a spread of queries that contains the planted ones, against all candidates: a query's answer does not depend
   on the other queries); the float64 restatements of
   sections E, F and G agree with the fp32 oracle functions to fp32 noise;
 - measured constants: recomputed here, 4 x noise <= tolerance;
 - input conditions: the pinned seeds are the first that meet their conditions (threshold margins, at least four valid
   pixels, well-conditioned cross-covariances), and the degenerate ICP inputs are degenerate."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import chamfer_ref as C
from oracle import frontend_ref as FR
from oracle import geometry_ref as G
from tests import test_gpu_eval_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _source(*path):
    return open(os.path.join(ROOT, *path)).read()


def launcher(text, name):
    """The body of `extern "C" int name(...)` with white space collapsed."""
    start = text.index('extern "C" int %s(' % name)
    end = text.find('\nextern "C"', start + 1)
    return re.sub(r"\s+", " ", text[start:end if end > 0 else len(text)])


def _int(pattern, src):
    found = re.findall(pattern, src)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


class Constants(object):
    """Read from the sources; the conditions around them are required verbatim, so a launcher that changes shape fails
    here instead of being restated wrongly."""

    def __init__(self):
        chamfer, grid_h = _source("zeroshape_amd", "csrc", "chamfer.hip"), _source("zeroshape_amd", "csrc", "zs_point_grid.h")
        pose, icp = _source("zeroshape_amd", "csrc", "pose_search.hip"), _source("zeroshape_amd", "csrc", "icp.hip")
        depth, plugin = _source("zeroshape_amd", "csrc", "depth_metrics.hip"), _source("zeroshape_amd", "chamfer_3D.py")
        self.src = {"zs_chamfer_forward": launcher(chamfer, "zs_chamfer_forward"),
                    "zs_chamfer_backward": launcher(chamfer, "zs_chamfer_backward"),
                    "zs_chamfer_forward_ws": launcher(_source("zeroshape_amd", "csrc", "chamfer_grid.hip"), "zs_chamfer_forward_ws"),
                    "zs_normalize_pc": launcher(pose, "zs_normalize_pc"), "zs_icp_step": launcher(icp, "zs_icp_step"),
                    "zs_standardize_pc": launcher(icp, "zs_standardize_pc"), "zs_depth_metrics": launcher(depth, "zs_depth_metrics")}

        def need(name, snippet):
            assert snippet in self.src[name], "%s no longer reads: %s" % (name, snippet)
        # brute scan
        self.nn_threads = _int(r"constexpr int NN_THREADS = (\d+);", chamfer)
        a, b = re.findall(r"const int Q = \(\(long long\)b \* nmax >= (\d+) \* (\d+)\) \? 2 : 1;", self.src["zs_chamfer_forward"])[0]
        self.q2_from = int(a) * int(b)
        self.batch_limit = _int(r"if \(b > (\d+)\) \{", self.src["zs_chamfer_forward"])
        assert _int(r"if \(b > (\d+)\) \{", self.src["zs_chamfer_forward_ws"]) == self.batch_limit
        need("zs_chamfer_forward", "dim3 grid((nmax + NN_THREADS * Q - 1) / (NN_THREADS * Q), b, 2);")
        need("zs_chamfer_forward", "hipLaunchKernelGGL(nn_both_sgpr_kernel<2>,")
        need("zs_chamfer_forward", "hipLaunchKernelGGL(nn_both_sgpr_kernel<1>,")
        for line in ("const int q_base = blockIdx.x * (NN_THREADS * Q);", "if (q_base >= n || m == 0) return;",
                     "j = j < n ? j : n - 1;", "const int m8 = m & ~7;", "for (; k + 16 <= m8; k += 16) {",
                     "if (k + 16 < m8) A.request_before(", "if (k < m8) scan8(A, k);", "for (int k = m8; k < m; k++) {"):
            assert line in chamfer, line
        # the plugin's method="auto"
        self.grid_min_points = _int(r"\nGRID_MIN_POINTS = (\d+)\n", plugin)
        assert 'use_grid = min(n, m) > 0 and (method == "grid" or (method == "auto" and max(n, m) >= GRID_MIN_POINTS))' in plugin
        # the grid
        self.grid_max_axis = _int(r"constexpr int GRID_MAX_AXIS = (\d+);", grid_h)
        self.per_cell = _int(r"while \(a < GRID_MAX_AXIS && \(long long\)\(a \+ 1\) \* \(a \+ 1\) \* \(a \+ 1\) \* (\d+) <= mc\) a\+\+;", grid_h)
        # backward
        self.bwd_threads = _int(r"int blocks = \(int\)\(\(nmax \+ 255\) / (\d+)\);", self.src["zs_chamfer_backward"])
        self.bwd_max_blocks = _int(r"if \(blocks > (\d+)\) blocks = \1;", self.src["zs_chamfer_backward"])
        need("zs_chamfer_backward", "const long long nmax = (long long)b * (n > m ? n : m);")
        need("zs_chamfer_backward", "dim3(blocks, 1, 2), dim3(%d)" % self.bwd_threads)
        # normalize_pc, standardize_pc, icp
        self.ps_threads = _int(r"constexpr int PS_THREADS = (\d+);", pose)
        need("zs_normalize_pc", "int bx = (n + PS_THREADS - 1) / PS_THREADS;")
        self.normalize_max_blocks = _int(r"if \(bx > (\d+)\) bx = \1;", self.src["zs_normalize_pc"])
        self.icp_threads = _int(r"constexpr int ICP_THREADS = (\d+);", icp)
        need("zs_icp_step", "int bx = (n + ICP_THREADS - 1) / ICP_THREADS;")
        self.icp_max_blocks = _int(r"if \(bx > (\d+)\) bx = \1;", self.src["zs_icp_step"])
        need("zs_icp_step", "hipLaunchKernelGGL(icp_fit_kernel, dim3(b), dim3(ICP_THREADS)")
        need("zs_standardize_pc", "hipLaunchKernelGGL(standardize_pc_kernel, dim3(b), dim3(ICP_THREADS)")
        # icp_fit_kernel: how u_i is formed from the i-th singular triplet
        arms = re.findall(r"if \(sv > (\S+) \* smax && sv > 0\.0\) \{.*?\} else if \(nrm > (\S+) \* smax && nrm > 0\.0\) \{.*?"
                          r"\} else if \(i == 2\) \{.*?\} else if \(i == 1\) \{.*?\} else \{", icp, flags=re.S)
        assert len(arms) == 1, arms
        self.icp_sv_from, self.icp_norm_from = float(arms[0][0]), float(arms[0][1])
        # depth metrics
        self.depth_block = _int(r"constexpr int BLOCK = (\d+);", depth)
        self.max_thr = _int(r"constexpr int MAX_THR = (\d+);", depth)
        need("zs_depth_metrics", "if (batch < 0 || n <= 0 || n_thresholds < 0 || n_thresholds > MAX_THR) {")
        need("zs_depth_metrics", "dim3(batch), dim3(BLOCK)")
        assert "for (int i = tid; i < n; i += BLOCK)" in depth

    def axis_cells(self, mc):
        a = 1
        while a < self.grid_max_axis and (a + 1) ** 3 * self.per_cell <= mc:
            a += 1
        return a


@pytest.fixture(scope="module")
def K():
    return Constants()


# =====================================================================================================
# branch accounting
# =====================================================================================================
def brute_branches(K, b, n, m):
    """The branches of zs_chamfer_forward / nn_both_sgpr_kernel one launch takes."""
    nmax = max(n, m)
    Q = 2 if b * nmax >= K.q2_from else 1
    out = {"Q%d" % Q}
    per_block = K.nn_threads * Q
    blocks = (nmax + per_block - 1) // per_block
    for queries, cands in ((n, m), (m, n)):
        own = (queries + per_block - 1) // per_block
        if own < blocks:
            out.add("Q%d block past the direction's queries returns" % Q)
        last = queries - (own - 1) * per_block                      # queries of the direction's last block
        for slot in range(Q):
            if own > 1:
                out.add("Q%d slot %d full" % (Q, slot))             # the blocks in front of the last one
            filled = min(max(last - slot * K.nn_threads, 0), K.nn_threads)
            out.add("Q%d slot %d %s" % (Q, slot, "full" if filled == K.nn_threads else "empty" if filled == 0 else "partial"))
        chunks, tail = cands // 8, cands % 8
        out.add("Q%d %s" % (Q, "no chunk" if chunks == 0 else "odd chunks" if chunks % 2 else "even chunks"))
        if chunks >= 3:
            out.add("Q%d chunk A requested again" % Q)
        out.add("Q%d %s" % (Q, "tail" if tail else "no tail"))
    if b == K.batch_limit:
        out.add("batch limit")
    return out


def test_brute_cases_reach_every_branch_of_both_instantiations(K):
    assert (K.nn_threads, K.q2_from, K.batch_limit) == (256, 65536, 65535)
    seen = {}
    for case in E.BRUTE_CASES + E.NONFINITE_CASES[:2]:
        for name in brute_branches(K, *case):
            seen.setdefault(name, []).append(case)
    for case in E.BRUTE_Q2:
        assert "Q2" in brute_branches(K, *case), case
    want = {"Q2", "Q2 block past the direction's queries returns", "Q2 slot 0 full", "Q2 slot 0 partial", "Q2 slot 1 full",
            "Q2 slot 1 partial", "Q2 slot 1 empty", "Q2 no chunk", "Q2 odd chunks", "Q2 even chunks", "Q2 chunk A requested again",
            "Q2 tail", "Q2 no tail", "batch limit", "Q1", "Q1 slot 0 full", "Q1 slot 0 partial", "Q1 odd chunks", "Q1 tail"}
    for name in sorted(want):
        print("%s: %s" % (name, seen.get(name, [])[:4]))
    assert want <= set(seen), sorted(want - set(seen))
    # the cases the issue names do what it says of them
    assert {"Q2 slot 1 empty", "Q2 block past the direction's queries returns"} <= brute_branches(K, 128, 513, 17)
    assert brute_branches(K, 128, 512, 512) == {"Q2", "Q2 slot 0 full", "Q2 slot 1 full", "Q2 even chunks", "Q2 chunk A requested again",
                                                "Q2 no tail"}
    assert "Q2 slot 1 partial" in brute_branches(K, 256, 257, 300)
    assert {"Q2 even chunks", "Q2 no tail", "Q2 tail"} <= brute_branches(K, 2048, 33, 32)
    assert {(m // 8, m % 8) for b, n, m in E.BRUTE_Q2 if b == 512} == {(c, t) for c in (1, 2, 3) for t in (0, 1, 7)} - {(3, 7)}
    # ... and again with live lanes in slot 1: there 130 queries leave it a repeat of the last query
    for b, n, m in E.BRUTE_LIVE_SLOT1:
        assert "Q2 slot 1 partial" in brute_branches(K, b, n, m) and "Q2 slot 1 partial" not in brute_branches(K, 512, 130, m)
    assert {m for _, _, m in E.BRUTE_LIVE_SLOT1} == {m for b, _, m in E.BRUTE_Q2 if b == 512}
    # both sides of the selector, one query apart
    (b0, n0, m0), (b1, n1, m1) = E.BRUTE_SELECTOR
    assert b0 * max(n0, m0) == K.q2_from and "Q2" in brute_branches(K, b0, n0, m0)
    assert b1 * max(n1, m1) == K.q2_from - b1 and "Q1" in brute_branches(K, b1, n1, m1)
    assert "Q1" in brute_branches(K, *E.NONFINITE_CASES[0]) and "Q2" in brute_branches(K, *E.NONFINITE_CASES[1])


def test_grid_cases_build_every_grid_size_on_both_sides_of_every_boundary(K):
    assert K.grid_max_axis == 16 and K.per_cell == 2
    boundaries = [K.per_cell * a ** 3 for a in range(2, K.grid_max_axis + 1)]     # the smallest cloud with a cells per axis
    assert boundaries == [16, 54, 128, 250, 432, 686, 1024, 1458, 2000, 2662, 3456, 4394, 5488, 6750, 8192]
    for a, mc in zip(range(2, K.grid_max_axis + 1), boundaries):
        assert K.axis_cells(mc - 1) == a - 1 and K.axis_cells(mc) == a
    sizes = {s for n, m, _ in E.GRID_CASES for s in (n, m)}                       # every cloud is a candidate set one way
    assert {K.axis_cells(s) for s in sizes} == set(range(1, K.grid_max_axis + 1))
    for mc in boundaries:
        assert mc - 1 in sizes and mc in sizes
    assert {1, 2, 3} <= sizes and K.axis_cells(10 ** 6) == K.grid_max_axis
    kinds = {}
    for n, m, kind in E.GRID_CASES:
        kinds.setdefault(kind, set()).update((K.axis_cells(n), K.axis_cells(m)))
    assert set(kinds) == {"uniform"} | set(E.GEOMETRIES)
    assert kinds["uniform"] == set(range(1, K.grid_max_axis + 1))
    for kind in E.GEOMETRIES:
        assert len(kinds[kind]) >= 2, kind
    assert min(n for n, m, _ in E.GRID_CASES) < K.grid_min_points                 # method="grid" forced below the auto threshold
    # method="auto" on both sides of GRID_MIN_POINTS
    assert sorted(max(n, m) for n, m in E.AUTO_PAIRS) == [K.grid_min_points - 1, K.grid_min_points]
    # the non-finite cases: <1>, <2> and two grids of different sizes
    assert {K.axis_cells(300), K.axis_cells(2000)} == {5, 10}


def test_grid_stride_loops_are_entered(K):
    # zs_chamfer_backward
    cap = K.bwd_max_blocks * K.bwd_threads
    assert (K.bwd_max_blocks, K.bwd_threads, cap) == (2048, 256, 524288)
    work = [b * max(n, m) for b, n, m, _ in E.BACKWARD_CASES]
    assert max(work) == 550000 and cap < max(work) < 2 * cap and min(work) == 2      # the loop wraps once; one block
    assert any(kind == "one" for _, _, _, kind in E.BACKWARD_CASES)
    # zs_normalize_pc's apply pass and zs_icp_step's
    for threads, blocks, sizes in ((K.ps_threads, K.normalize_max_blocks, E.PC_SIZES),
                                   (K.icp_threads, K.icp_max_blocks, [n for n, _ in E.ICP_CASES])):
        assert (threads, blocks) == (256, 64)
        cap = threads * blocks
        assert any(cap < s < 2 * cap for s in sizes) and any(s <= cap for s in sizes)
        assert any(s < threads for s in sizes) and any(s % threads for s in sizes if s > threads)
    assert {63, 64, 65, 255, 256, 257, 16384, 16385, 16641} <= set(E.PC_SIZES) and 16641 == 65 * 256 + 1
    assert {n for n, _ in E.ICP_CASES} >= {255, 256, 257, 16385}


def test_depth_cases_cover_the_sweeps_and_the_threshold_counts(K):
    assert (K.depth_block, K.max_thr) == (1024, 8)
    pixels = sorted(H * W for H, W in E.DEPTH_MAPS)
    assert pixels == [1, 63, 65, 1023, 1024, 1025, 2240]
    assert K.depth_block - 1 in pixels and K.depth_block in pixels and K.depth_block + 1 in pixels
    assert any(p > 2 * K.depth_block and p % K.depth_block for p in pixels)          # a third, ragged sweep
    assert sorted(E.DEPTH_THRESHOLDS) == [0, 3, K.max_thr] and all(len(v) == k for k, v in E.DEPTH_THRESHOLDS.items())
    assert sorted(E.DEPTH_OPTIONS, key=str) == sorted([("depth", None), ("depth", 1.5), ("disparity", None), ("disparity", 1.5)], key=str)


# =====================================================================================================
# references
# =====================================================================================================
def _query_sample(size, planted, budget):
    if size <= budget:
        return np.arange(size)
    keep = set(np.linspace(0, size - 1, budget).astype(int).tolist()) | {j for j in planted if j < size}
    return np.array(sorted(keep))


def contract_equals_oracle(a, c, want, what, pairs):
    """nn_contract in every batch element, both directions: on all queries while a direction has at most `pairs` pairs, else
    on a spread of queries that contains the planted ones, against all candidates.  -> (queries checked, queries in all)."""
    b = a.shape[0]
    planted = (0, 7, 8, 11, 16, 100, a.shape[1] - 1, c.shape[1] - 1)
    checked = 0
    for q, k, d_w, i_w in ((a, c, want[0], want[2]), (c, a, want[1], want[3])):
        rows = _query_sample(q.shape[1], planted, max(8, pairs // (b * k.shape[1])))
        d, i = E.nn_contract(np.ascontiguousarray(q[:, rows]), k)
        E.same_bits(d, d_w[:, rows], what + " distances")
        E.same_bits(i, i_w[:, rows], what + " indices")
        checked += d.size
    return checked, want[0].size + want[1].size


def test_contract_restatement_equals_the_oracle_on_finite_and_infinite_input():
    total, sampled = 0, []
    for case in E.BRUTE_CASES:
        a, c = E.brute_clouds(*case)
        assert not np.isnan(a).any() and not np.isnan(c).any()
        if min(case[1:]) >= 17:
            assert np.isinf(a).any() and np.isinf(c).any()
        done, of = contract_equals_oracle(a, c, C.chamfer_forward(a, c), "A %s" % (case,), pairs=4 << 20)
        total += done
        if done < of:
            sampled.append(case)
    assert sampled == [(128, 512, 512), (256, 257, 300)]        # every other case of A: all queries of all batch elements
    for case in E.GRID_CASES:
        a, c = E.grid_clouds(*case)
        assert np.isfinite(a).all() and np.isfinite(c).all()
        done, of = contract_equals_oracle(a, c, E.grid_oracle(*case), "B %s" % (case,), pairs=1 << 18)
        total += done
        assert done == of or max(case[:2]) > 360                # below that: all queries
    print("the contract's restatement equals the oracle on %d queries" % total)


def test_grid_geometries_are_what_they_are_called():
    a, c = E.grid_clouds(2661, 2662, "tiny")
    d1 = E.grid_oracle(2661, 2662, "tiny")[0]
    assert float(d1.max()) < float(np.finfo(F32).tiny) and int((d1 == 0).sum()) >= 2        # subnormal distances and zeros
    a, c = E.grid_clouds(1457, 1458, "shift1e5")
    assert len(np.unique(a[..., 0])) <= 129                                                 # 2^-7 is the spacing at 1e5
    a, c = E.grid_clouds(5487, 5488, "lattice")
    assert len(np.unique(c.reshape(-1, 3), axis=0)) <= 729
    a, c = E.grid_clouds(1999, 2000, "flat")
    assert np.ptp(c[..., 2]) == 0 and np.ptp(np.delete(a[0, :, 0], 11)) == 0                # (point 11 is a planted duplicate)
    a, c = E.grid_clouds(3455, 3456, "huge")
    assert np.isfinite(E.grid_oracle(3455, 3456, "huge")[0]).all() and float(np.abs(c).max()) > 1e14
    a, c = E.grid_clouds(6749, 6750, "shell")
    d1 = E.grid_oracle(6749, 6750, "shell")[0]                                              # direction 0: shell -> cluster
    assert float(np.abs(np.linalg.norm(c, axis=-1) - 1).max()) < 1e-6 and float(np.abs(np.delete(a, 11, axis=1)).max()) < 0.01
    for kind in ("uniform",) + tuple(E.GEOMETRIES):
        n, m = next((n, m) for n, m, k in E.GRID_CASES if k == kind and m > 100)
        a, c = E.grid_clouds(n, m, kind)
        assert np.array_equal(c[:, 100], c[:, 7]) and np.array_equal(a[:, 11], c[:, 7])
        assert np.all(E.grid_oracle(n, m, kind)[2][:, 11] <= 7)                             # never 100: the lowest index wins


def test_non_finite_cases_hold_what_the_contract_speaks_of():
    assert [p[:3] for p in E.NONFINITE_PARAMS if p[3] == 0] == E.NONFINITE_CASES               # the issue's four, and
    assert [p[:3] for p in E.NONFINITE_PARAMS if p[3] != 0] == E.NONFINITE_CASES[2:]           # the grid's two again, moved
    for b, n, m, shift in E.NONFINITE_PARAMS:
        a, c = E.nonfinite_clouds(b, n, m, shift)
        if shift:                                        # across a power of two, far from the origin against the extent
            fin = a[np.isfinite(a) & (a != 0)]           # (one planted point is (+inf, -inf, 0))
            assert shift == 1024 and fin.min() < 1024 < fin.max() and np.ptp(fin) <= 1.0
            assert np.spacing(F32(1023.9)) * 2 == np.spacing(F32(1024.1)) and np.isinf(a[0]).any() and np.isinf(c[0]).any()
        assert np.isnan(c[b - 1]).all() and not np.isnan(a[b - 1]).all()
        for x in (a, c):
            assert np.isnan(x[0, 0, 0]) and np.isnan(x[0, 8, 2]) and np.isnan(x[0, -1, 1])
            assert np.all(x[0, 3] == np.inf) and x[0, 5, 0] == -np.inf
        d1, d2, i1, i2 = E.contract_forward(a, c)
        for d, i in ((d1, i1), (d2, i2)):
            assert not np.isnan(d).any() and np.all(i[np.isinf(d)] == 0) and np.all(d >= 0)
        assert np.isinf(d1[0, 0]) and np.isinf(d2[0, 0])                                    # NaN queries
        # the oracle disagrees exactly where the contract says it does: NaN in candidate 0 or in the query
        o1 = C.chamfer_forward(a, c)[0]
        assert np.isnan(o1[0]).all() and np.isfinite(d1[0, 1]) and d1[0, 1] > 0
        assert bool(np.isfinite(d1[0]).sum() >= n - 8)


def test_fscore_oracle_counts_with_a_strict_comparison_in_fp32():
    for n, m in E.FSCORE_SIZES:
        for nt, thr in E.FSCORE_THRESHOLDS.items():
            d1, d2 = E.fscore_inputs(n, m, nt)
            want = G.compute_fscore(torch.from_numpy(d1), torch.from_numpy(d2), thr).numpy()
            t32 = np.array(thr, F32)
            p = (d1[:, :, None] < t32).sum(1).astype(F32) / F32(n)
            r = (d2[:, :, None] < t32).sum(1).astype(F32) / F32(m)
            with np.errstate(invalid="ignore"):
                f = F32(2) * p * r / (p + r)
            f[np.isnan(f)] = 0
            E.same_bits(want, f.astype(F32), "fscore oracle (%d, %d, %d)" % (n, m, nt))
            assert np.all(want[2] == 0)
            assert any(np.any(x[:2] == t) for x in (d1, d2) for t in t32)                   # equal to a threshold somewhere
            if min(n, m) > 5:
                assert np.isnan(d1[0]).sum() == 2 and np.isnan(d2[0]).sum() == 2
                # counting the equal ones would change the answer: the strict comparison is tested
                p2 = (d1[:, :, None] <= t32).sum(1).astype(F32) / F32(n)
                assert not np.array_equal(p, p2)


def test_icp_reference_agrees_with_the_fp32_oracle_and_inputs_are_conditioned():
    for n, m in E.ICP_CASES:
        assert E.icp_seed_search(n, m) == E.ICP_SEEDS[(n, m)]
        x1, x2 = E.icp_clouds(n, m)
        S, dets = E.icp_singular_values(x1, x2)
        print("ICP (%d, %d): singular values over the largest %s, det(V U^T) %s"
              % (n, m, np.array2string(S, precision=3).replace("\n", ""), np.array2string(dets, precision=2)))
        idx = C.chamfer_forward(x1, x2)[2]
        for i in range(E.ICP_B):
            t1, t2, _, cands = E.icp_reference(x1[i], x2[i], idx[i])
            for R, _ in cands:
                assert abs(np.linalg.det(R) - 1) < 1e-12 and float(np.abs(R @ R.T - np.eye(3)).max()) < 1e-12
            if (n, m) in E.ICP_RANK2:
                assert S[i, 1] >= 0.05 and S[i, 2] <= 1e-6
                assert float(np.abs(cands[0][0] - cands[1][0]).max()) > 0.1                 # two different answers
            else:
                assert S[i, 2] >= 1e-3
                want = G.icp(torch.from_numpy(x1[i:i + 1].copy()), torch.from_numpy(x2[i:i + 1].copy()), 1)[0].numpy()
                err = float(np.abs(want - cands[0][1]).max())
                assert err < 1e-5, (n, m, i, err)                                           # torch.svd on an fp32 matrix
        if (n, m) not in E.ICP_RANK2:
            assert dets[2] < 0 < min(dets[0], dets[1]) and n >= 255                         # the mirrored cloud: the row rule acts
    assert abs(np.arccos((np.trace(E._rotation([2, -1, 1], 2.5)) - 1) / 2) - 2.5) < 1e-12


def fit_arms(K, S):
    """The arm of icp_fit_kernel each singular triplet takes, from the singular values over the largest (float64 SVD).  The
    kernel decides on sqrt(eigenvalue of H^T H) and on |H v_i|, which agree with the true values to ~1e-8 and ~1e-15 of the
    largest: the restatement holds for values a factor 2 away from both thresholds and, where they vanish, below 1e-10."""
    out = []
    for i, s in enumerate(S):
        assert i == 0 or s <= 1e-10 or min(abs(np.log(s / t)) for t in (K.icp_sv_from, K.icp_norm_from)) > np.log(2), (i, s)
        if S[0] > 0 and s > K.icp_sv_from:
            out.append("H v / s")
        elif S[0] > 0 and s > K.icp_norm_from:
            out.append("H v / |H v|")
        else:
            out.append("completed %d" % i)
    return tuple(out)


def test_icp_cases_reach_every_arm_of_the_fit(K):
    assert (K.icp_sv_from, K.icp_norm_from) == (1e-4, 1e-6)
    seen = {}
    cases = [("(%d, %d)" % c, E.icp_clouds(*c)) for c in E.ICP_CASES]
    cases += [("slab %s" % kind, E.icp_slab_clouds(kind)) for kind in sorted(E.ICP_SLAB_WINDOWS)]
    cases += [(kind, E.icp_degenerate_clouds(kind)) for kind in E.ICP_DEGENERATE if kind != "coincident"]   # (its H is noise)
    for name, (x1, x2) in cases:
        S, det = E.icp_singular_values(x1, x2)
        arms = {fit_arms(K, s) for s in S}
        assert len(arms) == 1, (name, arms)
        seen[name] = arms.pop()
        print("ICP %s: %s" % (name, ", ".join(seen[name])))
    full = ("H v / s",) * 3
    for c in E.ICP_CASES:
        assert seen["(%d, %d)" % c] == (full if c not in E.ICP_RANK2 else full[:2] + ("completed 2",))
    assert seen["slab sv"] == full and seen["slab norm"] == full[:2] + ("H v / |H v|",)
    assert seen["line"] == ("H v / s", "completed 1", "completed 2")
    assert seen["one_point"] == ("completed 0", "completed 1", "completed 2")
    assert {a for arms in seen.values() for a in arms} == {"H v / s", "H v / |H v|", "completed 0", "completed 1", "completed 2"}
    # the slab cases: the first seeds inside their windows, on the two sides of the threshold, R unique (a rotation, with
    # the row rule acting on the mirrored cloud)
    lo, hi = E.ICP_SLAB_WINDOWS["norm"], E.ICP_SLAB_WINDOWS["sv"]
    assert K.icp_norm_from * 2 < lo[0] and lo[1] * 2 < K.icp_sv_from and K.icp_sv_from * 2 <= hi[0] and hi[1] < 1e-3
    for kind in sorted(E.ICP_SLAB_WINDOWS):
        assert E.icp_slab_seed_search(kind) == E.ICP_SLAB_SEEDS[kind]
        x1, x2 = E.icp_slab_clouds(kind)
        S, det = E.icp_singular_values(x1, x2)
        w_lo, w_hi = E.ICP_SLAB_WINDOWS[kind]
        assert np.all(S[:, 2] >= w_lo) and np.all(S[:, 2] <= w_hi) and np.all(S[:, 1] >= 0.1) and det[2] < 0 < min(det[0], det[1])
        idx = C.chamfer_forward(x1, x2)[2]
        for i in range(E.ICP_B):
            R = E.icp_reference(x1[i], x2[i], idx[i])[3][0][0]
            assert abs(np.linalg.det(R) - 1) < 1e-12 and float(np.abs(R @ R.T - np.eye(3)).max()) < 1e-12


def test_degenerate_icp_inputs_are_degenerate():
    for kind in E.ICP_DEGENERATE:
        x1, x2 = E.icp_degenerate_clouds(kind)
        idx = C.chamfer_forward(x1, x2)[2]
        for i in range(E.ICP_B):
            H = E.icp_cross_covariance(x1[i], x2[i], idx[i])[2]
            S = np.linalg.svd(H, compute_uv=False)
            if kind == "one_point":
                assert x1.shape[1] == 1 and np.all(H == 0)
            elif kind == "coincident":
                assert np.all(x1[i] == x1[i, 0]) and S[0] < 1e-9
            else:
                d = x1[i].astype(F64) - x1[i, 0].astype(F64)
                assert np.all(np.cross(d, np.array([1.0, 2.0, -1.0])) == 0) and np.ptp(d[:, 0]) > 0.5    # exactly on one line
                assert S[0] > 1e-3 and S[1] <= 1e-12 * S[0]


def test_depth_reference_agrees_with_the_fp32_oracle_and_inputs_meet_their_conditions():
    worst = 0.0
    for H, W in E.DEPTH_MAPS:
        assert E.depth_seed_search(H, W) == E.DEPTH_SEEDS[(H, W)]
        pred, target, mask = E.depth_inputs(H, W)
        valid = mask.sum((1, 2, 3))
        assert int(valid[1]) == 0
        if H * W == 1:
            assert int(valid[0]) == int(valid[2]) == 1
            for ptype, cap in E.DEPTH_OPTIONS:                      # one pixel: det = 0, (0, 0), +inf or the cap
                _, d, _, _ = E.depth_reference(E.depth_prediction(pred, ptype), target, mask, [], cap, ptype)
                assert np.all(d == (np.inf if cap is None else cap))
            continue
        assert int(min(valid[0], valid[2])) >= 4 and int(max(valid[0], valid[2])) < H * W
        e_valid, e_depth, e_metric = E.depth_oracle_noise(pred, target, mask)
        margin = E.depth_margin(pred, target, mask)
        print("depth (%d, %d): fp32 oracle %.2e on valid pixels, %.2e on all, %.2e on the metrics; margin %.2e"
              % (H, W, e_valid, e_depth, e_metric, margin))
        assert margin > 10 * e_valid and max(e_depth, e_metric) <= E.DEPTH_NOISE_MAX
        # the oracle's own threshold counts on these inputs equal the float64 ones (the margin at work)
        for ptype, cap in E.DEPTH_OPTIONS:
            p = E.depth_prediction(pred, ptype)
            thr = E.DEPTH_THRESHOLDS[8]
            want = E.depth_reference(p, target, mask, thr, cap, ptype)[0]
            om, _ = FR.depth_metrics(p, target, mask, thresholds=thr, depth_cap=cap, prediction_type=ptype)
            got = np.stack([om[k].numpy() for k in om], 1)
            n_valid = valid.numpy()[[0, 2], None]
            assert np.array_equal(np.rint(got[[0, 2], :8] * n_valid), np.rint(want[[0, 2], :8] * n_valid))
            assert np.all(np.isnan(got[1])) and np.all(np.isnan(want[1]))
        # compute_scale_and_shift's inputs: sample 1 keeps one pixel
        sp, st, sm = E.solve_inputs(H, W)
        assert int(sm[1].sum()) == 1
        B = sp.shape[0]
        want = np.stack(E.scale_shift_reference(*[x.numpy().astype(F64).reshape(B, -1) for x in (sp, st, sm)]), 1)
        got = torch.stack(FR.scale_and_shift(sp, st, sm.long()), 1).numpy()
        assert np.all(want[1] == 0) and np.all(got[1] == 0)
        worst = max(worst, e_depth, e_metric, E.rel_error(got, want))
    print("depth: fp32 oracle against float64 %.2e at the worst, tolerance %.1e" % (worst, E.DEPTH_RTOL))
    # the rule's value, nothing on top: max(the table's, 4 x noise), the noise term rounded up by 5 % at the most
    assert max(E.DEPTH_RTOL_TABLE, 4 * worst) <= E.DEPTH_RTOL <= max(E.DEPTH_RTOL_TABLE, 4.2 * worst)


# =====================================================================================================
# measured constants
# =====================================================================================================
def test_measured_constants_cover_four_times_the_fp32_noise():
    worst_n = worst_s = 0.0
    for n in E.PC_SIZES:
        x = E.pc_cloud(n)
        X = torch.from_numpy(x)
        worst_n = max(worst_n, E.allowance_units(G.normalize_pc(X).numpy(), E.normalize_reference(x), E.NORMALIZE_RTOL, E.NORMALIZE_ATOL))
        worst_s = max(worst_s, E.allowance_units(G.standardize_pc(X).numpy(), E.standardize_reference(x), 0.0, E.STANDARDIZE_ATOL))
        if n == 1:
            assert np.all(E.normalize_reference(x) == 0) and np.all(np.isnan(E.standardize_reference(x)))
    for what, noise, units in (("normalize_pc", worst_n, E.NORMALIZE_UNITS), ("standardize_pc", worst_s, E.STANDARDIZE_UNITS)):
        print("%s: fp32 oracle %.3f allowances off float64, tolerance %.2f allowances" % (what, noise, units))
        assert max(1.0, 4 * noise) <= units <= max(1.0, 4.2 * noise), what           # the rule's value, nothing on top
    # per batch element another scale and offset
    x = E.pc_cloud(257).astype(F64)
    assert len({round(float(s), 3) for s in x.std(axis=(1, 2))}) == E.PC_B and float(np.abs(x.mean(axis=1)).max()) > 5
    # section D's bound is a derivation, not a measurement: two roundings per term, k - 1 additions, one unit of room
    s, k = np.array([1.0]), np.array([5.0])
    assert float(E.backward_bound(s, k)[0]) == (5 + 3) * 2.0 ** -24
    # section F's are the issue's
    assert (E.ICP_T_ULP, E.ICP_R_ABS, E.ICP_OUT_ULP) == (1.0, 2.0 ** -23, 6.0)
