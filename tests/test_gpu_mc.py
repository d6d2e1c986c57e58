"""GPU parity: marching cubes + surface sampling kernels vs oracle/mc_ref.py (same tables,
same operation order): triangles and sampled points bit-exact.

The grids here are SMALL.  A unit of the count pass is one wave of 256 virtual cubes (a k-row of C = G - 1 cubes padded
to per_row = a multiple of 4) and a scan tile holds 2,048 units, so what each size reaches is:

    G    per_row  units  what it runs
    2    4         1     one live lane, 3 padding cubes; the row's fifth value from the extra load at the row's end
    3    4         1     four rows in one wave, every live lane at a row's end, 2 padding cubes
    9    8         2     one count block (4 units each), two lanes per row
    12   12        6     two count blocks, a partial last unit, 1 padding cube
    17   16       16     a wave spans 16 rows, no padding
    23   24       46     12 count blocks, a partial last unit, 2 padding cubes
    33   32      128     a wave spans 8 rows, no padding
    41   40      250     the largest here: 63 count blocks, ONE scan tile (mc_scan_offsets_kernel with blockIdx.x = 0)

all through mc_count_kernel<false>, one scan tile, and sampling over one tile (1,388 triangles).  Several scan tiles, the
row-per-wave kernel (G = 254 .. 257), sampling and mesh stats on production-size soups: tests/test_gpu_mc_full_size.py."""
import numpy as np
import pytest
import torch

from oracle import mc_ref as M
from tests.test_oracle_mc import _sphere

pytestmark = pytest.mark.gpu


def _noise_vol(G, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 1, (G, G, G)).astype(np.float32)       # every case, incl. ambiguous ones


@pytest.mark.parametrize("G,kind", [(2, "noise"), (3, "noise"), (9, "noise"), (17, "sphere"), (12, "noise"), (23, "noise"), (33, "sphere"),
                                    (41, "noise")])
def test_triangles_bit_exact(G, kind):
    from zeroshape_amd.utils import eval_3D as E
    vol = _noise_vol(G, G) if kind == "noise" else _sphere(G, 0.8)[0]
    scale = np.float32(3.0 / G)
    want = M.marching_cubes(vol, 0.5, scale, -1.5)
    tris, _ = E.extract_surface(torch.from_numpy(vol).cuda(), 0.5, -1.5, 1.5)
    got = tris.cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_empty_and_full_volumes():
    from zeroshape_amd.utils import eval_3D as E
    for val in (0.0, 1.0):
        tris, pts = E.extract_surface(torch.full((8, 8, 8), val).cuda(), 0.5, -1.5, 1.5, num_points=16)
        assert tris.shape == (0, 3, 3)
        assert pts.shape == (16, 3) and not bool(pts.any())       # utils/eval_3D.py:262


def test_sampling_matches_oracle():
    from zeroshape_amd.utils import eval_3D as E
    vol = _sphere(21, 0.9)[0]
    tris, pts = E.extract_surface(torch.from_numpy(vol).cuda(), 0.5, -1.5, 1.5, num_points=3000, seed=11)
    # bit for bit the oracle's point; a target on a cumulative-area boundary may pick the neighbouring triangle, then the
    # point is the oracle's formula on that neighbour, and at most 0.1 % of the rows may be such (check_cloud)
    from tests.test_gpu_mc_full_size import check_cloud
    assert tris.shape[0] == 1388
    check_cloud(tris.cpu().numpy(), pts.cpu().numpy(), 11, "sphere, G = 21")


def test_convert_to_explicit_contract_and_full_size():
    """reference signature: (meshes, pointclouds [B,10000,3] float64); 129^3 grid from the decoder
    path: cloud lies on the level set of the trilinear field within a voxel."""
    from zeroshape_amd.utils import eval_3D as E
    from zeroshape_amd.utils.options import EasyDict as edict
    opt = edict(dict(device="cuda", eval=dict(range=[-1.5, 1.5], num_points=10000)))
    G = 129
    vol = torch.from_numpy(_sphere(G, 1.0, c=(0, 0, 0))[0]).cuda()
    meshes, clouds = E.convert_to_explicit(opt, [vol, vol.cpu().numpy()], isoval=0.5, to_pointcloud=True)
    assert len(meshes) == 2 and clouds.shape == (2, 10000, 3) and clouds.dtype == np.float64
    # the indexed form of mcubes.marching_cubes (utils/eval_3D.py:250-256): welded vertices, the triangle set unchanged
    m = meshes[0]
    assert m.faces.shape[1] == 3 and len(m.faces) == len(m.triangles)
    assert len(np.unique(m.vertices.view(np.uint32), axis=0)) == len(m.vertices) < 3 * len(m.faces)
    assert np.array_equal(m.vertices[m.faces].view(np.uint32), (m.triangles + np.float32(0)).view(np.uint32))
    assert len(m.vertices) - 3 * len(m.faces) // 2 + len(m.faces) in (2, 0, 4)      # Euler characteristic of a closed surface (V - E + F, E = 3F/2)
    # world coordinates use the reference's S = G scaling: radius 1.0 * (G-1)/G, centre -1.5/G
    r = np.linalg.norm(clouds[0] - (-1.5 / G), axis=1)
    assert abs(r.mean() - (G - 1) / G) < 2e-3 and r.std() < 2e-3
    assert not np.array_equal(clouds[0], clouds[1])      # different seeds per grid index
