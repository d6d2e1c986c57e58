"""GPU parity at the grid sizes evaluation runs (129^3, 257^3): marching cubes, surface sampling and - from
tests/test_gpu_render.py - mesh stats on the launch paths only such sizes reach, against oracle/mc_ref.py.

Which path a grid size G takes (C = G - 1 cubes per row, per_row = C rounded up to a multiple of 4 virtual cubes, a unit =
one wave = 256 virtual cubes, a scan tile = 2,048 units; the scan covers units + 1 entries):

    G        per_row  units    scan tiles  count kernel
    82       84        2,153    2          generic    first size with a second tile; 3 padding cubes per row
    83       84        2,207    2          generic    2 padding cubes
    129      128       8,192    5          generic    a wave spans two rows
    253      252      62,512   31          generic    the size below the row-per-wave ones, no padding
    254      256      64,009   32          ROWWAVE    a wave is one row; 3 padding cubes
    255      256      64,516   32          ROWWAVE    2 padding cubes
    256      256      65,025   32          ROWWAVE    1 padding cube
    257      256      65,536   33          ROWWAVE    no padding: the only size whose lane 63 feeds a live cube (k = 255)
                                                      with the row's last value, the wave-uniform load of load_cube_rows
    258      260      67,082   33          generic    the size above, 3 padding cubes

With more than one tile mc_scan_offsets_kernel runs with blockIdx.x > 0: the tile offset it adds, the active-unit list
index it takes from the high half and the totals it reads from the last tile are what these cases hold to the oracle.
zs_mesh_sample scans its cumulative areas over the same 2,048-entry tiles (the soups below: 1 to 864 tiles).

NOT tested: the 64-bit branch of virtual_ijk (2^31 virtual cubes or more) needs G >= 1292, a volume of 8.6 GB.

Every (volume, oracle soup, GPU soup) the triangle, sampling and stats tests share is computed once (`case`)."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from oracle import mc_ref as M
from tests.test_oracle_mc import (WIDE_ISO, WIDE_RANGE, _field_f, _noise, _non_finite, _sphere, _three_valued, _wide_range,
                                  soup_cube_census)

pytestmark = pytest.mark.gpu

# name -> (volume, iso, (lo, hi))
VOLUMES = {
    "noise82": (lambda: _noise(82, 82), 0.5, (-1.5, 1.5)),
    "noise83": (lambda: _noise(83, 83), 0.5, (-1.5, 1.5)),
    "three83": (lambda: _three_valued(83, 83), 0.5, (-1.5, 1.5)),
    "sphere83": (lambda: _sphere(83, 0.8)[0], 0.5, (-1.5, 1.5)),
    "wide12": (lambda: _wide_range(12, 12), WIDE_ISO, WIDE_RANGE),
    "nonfinite9": (lambda: _non_finite(9, 9), 0.5, (-1.5, 1.5)),
}
VOLUMES.update({"F%d" % G: (functools.partial(_field_f, G), 0.5, (-1.5, 1.5)) for G in (129, 253, 254, 255, 256, 257, 258)})
KEPT = {}                                   # the cases more than one test reads stay; the other 257^3-sized ones are dropped after use
SHARED = ("noise83", "three83", "sphere83", "nonfinite9", "F129", "F257")


def case(name):
    """(volume fp32 numpy, oracle soup numpy, GPU soup) of VOLUMES[name]; nothing in it may be written to."""
    if name in KEPT:
        return KEPT[name]
    from zeroshape_amd.utils import eval_3D as E
    make, iso, (lo, hi) = VOLUMES[name]
    vol = make()
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        want = M.marching_cubes(vol, iso, np.float32((hi - lo) / vol.shape[0]), lo)
    t1 = time.perf_counter()
    got, _ = E.extract_surface(torch.from_numpy(vol).cuda(), iso, lo, hi)
    torch.cuda.synchronize()
    print("%s: oracle %.2f s, upload + extract_surface %.3f s" % (name, t1 - t0, time.perf_counter() - t1))
    if name in SHARED:
        KEPT[name] = (vol, want, got)
    return vol, want, got


def launch_path(G):
    """(units, scan tiles, count kernel is the row-per-wave one) - the arithmetic of csrc/marching_cubes.hip, restated."""
    C = G - 1
    per_row = (C + 3) // 4 * 4
    units = (C * C * per_row + 255) // 256
    return units, (units + 1 + 2047) // 2048, per_row == 256


def test_the_sizes_reach_the_paths_the_docstring_names():
    assert [launch_path(G) for G in (41, 82, 83, 129)] == [(250, 1, False), (2153, 2, False), (2207, 2, False), (8192, 5, False)]
    assert [launch_path(G) for G in range(253, 259)] == [(62512, 31, False), (64009, 32, True), (64516, 32, True),
                                                         (65025, 32, True), (65536, 33, True), (67082, 33, False)]


# ---- 1. triangles, bit for bit ----

@pytest.mark.parametrize("name", ["noise82", "noise83", "three83", "sphere83", "wide12", "F129", "F253", "F254", "F255", "F256",
                                  "F257", "F258"])
def test_triangles_bit_exact(name):
    vol, want, got = case(name)
    got = got.cpu().numpy()
    G = vol.shape[0]
    census = soup_cube_census(want, G, *VOLUMES[name][2])
    print("%s: G=%d units=%d tiles=%d rowwave=%s triangles=%d census=%s" % ((name, G) + launch_path(G) + (len(want), census)))
    if name != "sphere83":
        # the surface is where these sizes' kernels differ from the small grids': the last cube of a k-row, the grid's faces
        assert min(census.values()) > 0, census
    if name[0] == "F":
        assert census["row_end"] > 10000 * G // 129 and min(census.values()) > 1000 * G // 129, census
    if name == "three83":
        assert (M.triangle_areas(want) == 0).mean() > 0.1
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def _assert_equal_outside_nan(got, want):
    assert got.shape == want.shape                                  # the triangle counts
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_nan_and_infinities_in_the_volume():
    """A NaN corner is 'not below the level' on both sides, and the vertices of its edges are NaN; an infinite corner gives
    NaN (inf / inf) when it is the edge's low endpoint and the other endpoint's position (x / inf = 0) when it is not."""
    vol, want, got = case("nonfinite9")
    assert np.isnan(vol).sum() == 1 and np.isposinf(vol).sum() == 1 and np.isneginf(vol).sum() == 1
    # the oracle's own numbers (oracle/mc_ref.py on the host)
    assert (len(want), int(np.isnan(want).any(-1).sum()), int(np.isinf(want).sum())) == (1663, 41, 0)
    _assert_equal_outside_nan(got.cpu().numpy(), want)


def test_permuted_view_and_fp64_volume():
    """extract_surface materialises what it is given as contiguous fp32: a permuted (non-contiguous) view of the same values
    and their fp64 copy give the soup of the fp32 array."""
    from zeroshape_amd.utils import eval_3D as E
    for name in ("nonfinite9", "wide12"):
        vol, want, _ = case(name)
        _, iso, (lo, hi) = VOLUMES[name]
        view = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 0, 1))).cuda().permute(1, 2, 0)
        assert not view.is_contiguous() and torch.equal(view.cpu().view(torch.int32), torch.from_numpy(vol).view(torch.int32))
        _assert_equal_outside_nan(E.extract_surface(view, iso, lo, hi)[0].cpu().numpy(), want)
        wide = torch.from_numpy(vol.astype(np.float64)).cuda()
        _assert_equal_outside_nan(E.extract_surface(wide, iso, lo, hi)[0].cpu().numpy(), want)


# ---- the C ABI: a short output buffer, refusals ----

def _abi():
    from zeroshape_amd import _lib
    from zeroshape_amd.utils import eval_3D as E
    lib = _lib.load()
    tab, cnt, stride = E._mc_tables(torch.device("cuda", torch.cuda.current_device()))
    return _lib, lib, tab, cnt, stride


def _error_text(lib):
    return (lib.zs_last_error() or b"").decode(errors="replace")


def test_emit_into_a_shorter_buffer_writes_no_row_past_it():
    _lib, lib, tab, cnt, stride = _abi()
    vol_np, want, _ = case("noise83")
    G = vol_np.shape[0]
    vol = torch.from_numpy(vol_np).cuda()
    scratch = torch.empty(lib.zs_mc_scratch_bytes(G) // 8 + 1, dtype=torch.int64, device="cuda")
    total = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = _lib.current_stream_ptr(vol.device)
    _lib.check(lib.zs_mc_count(_lib.ptr(vol), G, 0.5, _lib.ptr(cnt), _lib.ptr(scratch), _lib.ptr(total), stream), "zs_mc_count")
    n = int(total.item())
    assert n == len(want) > 2048
    sentinel = np.float32(-7777.25)
    for n_tris in (n - 7, 1):
        out = torch.full((n, 3, 3), float(sentinel), dtype=torch.float32, device="cuda")
        _lib.check(lib.zs_mc_emit(_lib.ptr(vol), G, 0.5, _lib.ptr(tab), stride, _lib.ptr(cnt), _lib.ptr(scratch),
                                  float(np.float32(3.0 / G)), -1.5, _lib.ptr(out), n_tris, stream), "zs_mc_emit")
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:n_tris].view(np.uint32), want[:n_tris].view(np.uint32))
        assert (got[n_tris:] == sentinel).all()


def test_count_and_emit_refuse_bad_arguments():
    _lib, lib, tab, cnt, stride = _abi()
    G = 9
    vol = torch.from_numpy(_noise(G, G)).cuda()
    scratch = torch.empty(lib.zs_mc_scratch_bytes(G) // 8 + 2, dtype=torch.int64, device="cuda")
    total = torch.full((1,), -3, dtype=torch.int32, device="cuda")
    out = torch.zeros(8, 3, 3, device="cuda")
    stream = _lib.current_stream_ptr(vol.device)
    p = _lib.ptr
    off4 = ctypes.c_void_p(scratch.data_ptr() + 4)
    assert lib.zs_mc_scratch_bytes(1) == 0 and lib.zs_mc_scratch_bytes(2) > 0

    def count(vol_p=p(vol), g=G, scratch_p=p(scratch)):
        return lib.zs_mc_count(vol_p, g, 0.5, p(cnt), scratch_p, p(total), stream)

    def emit(vol_p=p(vol), g=G, n_tris=8):
        return lib.zs_mc_emit(vol_p, g, 0.5, p(tab), stride, p(cnt), p(scratch), 1.0, 0.0, p(out), n_tris, stream)

    for what, call, text in [("G = 1", lambda: count(g=1), "bad grid size 1"), ("G = 2049", lambda: count(g=2049), "bad grid size 2049"),
                             ("null vol", lambda: count(vol_p=None), "null pointer"),
                             ("scratch + 4 bytes", lambda: count(scratch_p=off4), "8-byte aligned"),
                             ("emit: G = 1", lambda: emit(g=1), "bad size"), ("emit: G = 2049", lambda: emit(g=2049), "bad size"),
                             ("emit: negative n_tris", lambda: emit(n_tris=-1), "n_tris=-1"),
                             ("emit: null vol", lambda: emit(vol_p=None), "null pointer")]:
        assert call() == 0, what
        assert text in _error_text(lib), (what, _error_text(lib))
    torch.cuda.synchronize()
    assert int(total.item()) == -3 and not bool(out.any())             # a refused call launches nothing
    assert count() == 1 and emit(n_tris=0) == 1


# ---- 2. sampling over many scan tiles ----

SAMPLE_COUNTS = (1, 255, 256, 257, 10000)
SEEDS = (0, 11, 2 ** 63 + 5, 2 ** 64 - 1)


def _formula(p, r1, r2):
    """oracle/mc_ref.py's point of triangles p [n,3,3] at the (reflected) barycentric pair r1, r2."""
    return M._fma32(r2[:, None], p[:, 2] - p[:, 0], M._fma32(r1[:, None], p[:, 1] - p[:, 0], p[:, 0]))


def check_cloud(tris, got, seed, what):
    """Every row of `got` [n,3] (the GPU's cloud on the host soup `tris`) is, bit for bit, the oracle's point - or a
    BOUNDARY PICK: the oracle's formula, same r1 and r2, on the nearest triangle of non-zero area before or after the
    oracle's (the GPU adds the areas tile-wise, np.cumsum in index order: a target within an ulp of a cumulative boundary may
    land next door).  At most 0.1 % of the rows may be boundary picks; anything else fails.  -> their number."""
    n = len(got)
    want, ids = M.sample_surface(tris, n, seed)
    assert got.shape == want.shape == (n, 3) and got.dtype == np.float32
    same = (got.view(np.uint32) == want.view(np.uint32)).all(axis=1)
    odd = np.flatnonzero(~same)
    print("%s: %d samples on %d triangles (%d scan tiles), seed %d: %d boundary picks"
          % (what, n, len(tris), (len(tris) + 2047) // 2048, seed, len(odd)))
    if len(odd):
        s = odd.astype(np.uint64)
        r1, r2 = M._u01_many(seed, 3 * s + np.uint64(1)), M._u01_many(seed, 3 * s + np.uint64(2))
        flip = (r1 + r2).astype(np.float32) > np.float32(1.0)
        r1, r2 = np.where(flip, np.float32(1.0) - r1, r1).astype(np.float32), np.where(flip, np.float32(1.0) - r2, r2).astype(np.float32)
        np.testing.assert_array_equal(_formula(tris[ids[odd]], r1, r2), want[odd])         # the restatement is the oracle's
        solid = np.flatnonzero(M.triangle_areas(tris) > 0)
        before = np.searchsorted(solid, ids[odd], "left") - 1            # the last solid triangle before the oracle's ...
        after = np.searchsorted(solid, ids[odd], "right")                # ... and the first one after it, where there is one
        near = np.zeros(len(odd), bool)
        for at, there in ((before, before >= 0), (after, after < len(solid))):
            t = solid[np.clip(at, 0, len(solid) - 1)]
            near |= there & (_formula(tris[t], r1, r2).view(np.uint32) == got[odd].view(np.uint32)).all(axis=1)
        assert near.all(), "%s: rows %s are neither the oracle's point nor a neighbour's" % (what, odd[~near][:10].tolist())
    assert len(odd) <= 0.001 * n, "%s: %d boundary picks in %d samples" % (what, len(odd), n)
    return len(odd)


def _sample_soups():
    sphere = case("sphere83")[2]
    assert sphere.shape[0] == 18036
    soups = {"sphere83[:%d]" % k: sphere[:k] for k in (1, 2047, 2048, 2049)}
    soups.update({"sphere83": sphere, "F129": case("F129")[2], "F257": case("F257")[2], "three83": case("three83")[2]})
    return soups


SOUP_NAMES = ["sphere83[:1]", "sphere83[:2047]", "sphere83[:2048]", "sphere83[:2049]", "sphere83", "F129", "F257", "three83"]


@pytest.mark.parametrize("name", SOUP_NAMES)
def test_sampling_matches_oracle_on_many_tiles(name):
    from zeroshape_amd.utils import eval_3D as E
    soup = _sample_soups()[name]
    tris = soup.cpu().numpy()
    picks = 0
    for seed in SEEDS:
        for n in SAMPLE_COUNTS:
            got = E.sample_surface(soup, n, seed)
            assert got.shape == (n, 3) and got.dtype == torch.float32 and got.is_cuda
            picks += check_cloud(tris, got.cpu().numpy(), seed, name)
    print("%s: %d boundary picks in all" % (name, picks))
    if name == "three83":
        # the oracle never lands on a zero-area triangle (their cumulative area repeats the one before), so neither does a
        # GPU row that equals the oracle's
        area = M.triangle_areas(tris)
        assert 0.10 < (area == 0).mean() < 0.14
        for seed in SEEDS:
            assert (area[M.sample_surface(tris, 10000, seed)[1]] > 0).all()


def test_sampling_seeds_and_repeats():
    from zeroshape_amd.utils import eval_3D as E
    soup = case("F129")[2]
    bits = lambda seed, n=10000: E.sample_surface(soup, n, seed).cpu().numpy().view(np.uint32)      # noqa: E731
    a = bits(11)
    np.testing.assert_array_equal(bits(11), a)                           # the same seed, the same bits
    assert (bits(0) != a).any(axis=1).mean() > 0.99                      # another seed, another cloud
    np.testing.assert_array_equal(bits(-1), bits(2 ** 64 - 1))           # the wrapper masks the seed to 64 bits
    np.testing.assert_array_equal(bits(2 ** 64 + 11), a)


def test_sampling_of_nothing_and_from_the_host():
    from zeroshape_amd.utils import eval_3D as E
    soup = case("sphere83")[2]
    pts = E.sample_surface(soup[:0], 300, 5)
    assert pts.shape == (300, 3) and pts.is_cuda and not bool(pts.any())              # an empty soup gives zeros
    assert E.sample_surface(soup, 0, 5).shape == (0, 3)
    with pytest.raises(ValueError):
        E.sample_surface(soup.cpu(), 10, 5)
    with pytest.raises(ValueError):
        E.sample_surface(soup.cpu().numpy(), 10, 5)
