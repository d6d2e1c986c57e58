"""GPU: the weld and vertex-normal kernels (csrc/mesh_weld.hip) against SimpleMesh's numpy weld - vertices bit for bit, faces
and the vertex count equal - and against the numpy float64 restatement of the normals (eval_3D.vertex_normals_host), on
marching-cubes soups with every case, coincident vertices from different edges and zero-area triangles, on hand-written
soups, and through convert_to_explicit / dump_meshes / visualize_mesh."""
import functools

import numpy as np
import pytest
import torch

from tests.test_oracle_mc import _sphere
from zeroshape_amd.utils import eval_3D as E
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.options import EasyDict as edict

pytestmark = pytest.mark.gpu

# One fp32 rounding of a unit vector's component costs at most 2^-24 = 6e-8; the sum runs in the same order in fp64 on both
# sides, so what is left is sqrt / divide differences: 1e-6 absolute is margin.
NORMAL_ATOL = 1e-6

CASES = ["noise2", "noise3", "noise9", "noise23", "sphere33", "three_valued", "noise45"]


def _volume(name):
    if name.startswith("noise"):
        G = int(name[5:])
        return np.random.RandomState(G).uniform(0, 1, (G, G, G)).astype(np.float32)
    if name == "sphere33":
        return _sphere(33, 0.8)[0]
    assert name == "three_valued"                  # corner values ON the iso level: vertices of different edges coincide
    return np.random.RandomState(5).choice([0, 0.5, 1], (9, 9, 9)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(soup on the GPU, the numpy weld of its host copy, the numpy normals) - computed once, read by every test."""
    tris, _ = E.extract_surface(torch.from_numpy(_volume(name)).cuda(), 0.5, -1.5, 1.5)
    ref = E.SimpleMesh(tris.cpu().numpy())
    assert ref.device_triangles is None
    return tris, ref, ref.vertex_normals


def _assert_weld_equals(got_v, got_f, ref):
    assert got_v.dtype == torch.float32 and got_f.dtype == torch.int32 and got_v.is_cuda and got_f.is_cuda
    v, f = got_v.cpu().numpy(), got_f.cpu().numpy()
    assert v.shape == ref.vertices.shape, (v.shape, ref.vertices.shape)           # the vertex count
    assert f.shape == ref.faces.shape
    assert np.array_equal(v.view(np.uint32), ref.vertices.view(np.uint32))
    assert np.array_equal(f, ref.faces)


def _assert_normals_equal(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    zero = ~want.any(axis=1)
    assert not got[zero].any()                                                  # a zero sum: exactly (0, 0, 0)
    assert np.array_equal(~got.any(axis=1), zero)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max() if len(got) else 0.0
    print("normals: %d vertices, %d zero, max abs error %.3g" % (len(got), int(zero.sum()), err))
    assert err <= NORMAL_ATOL
    length = np.linalg.norm(got[~zero].astype(np.float64), axis=1)
    assert np.all(np.abs(length - 1.0) < 1e-6)


@pytest.mark.parametrize("name", CASES)
def test_weld_equals_the_numpy_weld(name):
    tris, ref, _ = _case(name)
    _assert_weld_equals(*E.weld_mesh(tris), ref)
    if name == "three_valued":
        t = ref.triangles.astype(np.float64)
        area2 = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
        # vertices ON grid corners (reached from every edge that ends there): all three coordinates are, to the bit, the
        # coordinate index * scale + offset of a grid plane
        planes = np.arange(9, dtype=np.float32) * np.float32(3.0 / 9) + np.float32(-1.5)
        on_corner = np.isin(ref.vertices, planes).all(axis=1)
        # (checked against oracle/mc_ref.py on the host: the same counts)
        assert (len(ref.triangles), len(ref.vertices), int(on_corner.sum()), int((area2 == 0).sum())) == (1156, 594, 29, 141)


@pytest.mark.parametrize("name", CASES)
def test_normals_equal_the_numpy_restatement(name):
    tris, ref, want = _case(name)
    v, f, n = E.weld_mesh(tris, normals=True)
    _assert_weld_equals(v, f, ref)                                              # the same weld with the normals asked for
    _assert_normals_equal(n, want)


def test_signed_zeros_are_one_vertex_and_keep_their_first_bits():
    soup = np.array([[[0, -0.0, 1], [1, 0, 0], [0, 1, 0]],
                     [[-0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]], np.float32)
    ref = E.SimpleMesh(soup)
    v, f, n = E.weld_mesh(torch.from_numpy(soup).cuda(), normals=True)
    _assert_weld_equals(v, f, ref)
    _assert_normals_equal(n, ref.vertex_normals)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert len(v) == 4 and f.tolist() == [[0, 2, 1], [0, 1, 3]]
    # vertex 0 = (0, -0, 1) of the first triangle, not the (-0, 0, 1) of the second
    assert v[0].view(np.uint32).tolist() == [0x00000000, 0x80000000, 0x3F800000]
    assert v[3].tolist() == [-1, 0, 0]                     # negative coordinates sort after positive ones: unsigned keys


def test_degenerate_sizes():
    dev = torch.device("cuda")
    for normals in (False, True):
        out = E.weld_mesh(torch.zeros(0, 3, 3, device=dev), normals=normals)
        assert [tuple(t.shape) for t in out] == [(0, 3)] * (3 if normals else 2)
        assert [t.dtype for t in out] == [torch.float32, torch.int32] + [torch.float32] * normals
        assert all(t.is_cuda for t in out)
    empty = E.SimpleMesh(torch.zeros(0, 3, 3, device=dev))
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.vertex_normals.shape == (0, 3)
    assert empty.vertices.dtype == np.float32 and empty.faces.dtype == np.int64 and empty.triangles.shape == (0, 3, 3)
    one = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    v, f, n = E.weld_mesh(torch.from_numpy(one).cuda(), normals=True)
    assert v.shape == (3, 3) and f.shape == (1, 3)
    _assert_weld_equals(v, f, E.SimpleMesh(one))
    assert n.cpu().numpy().tolist() == [[0, 0, 1]] * 3
    # a triangle whose three corners are one point: one vertex, no normal
    point = np.full((1, 3, 3), 0.25, np.float32)
    v, f, n = E.weld_mesh(torch.from_numpy(point).cuda(), normals=True)
    assert v.cpu().numpy().tolist() == [[0.25] * 3] and f.cpu().numpy().tolist() == [[0, 0, 0]] and not bool(n.any())
    with pytest.raises(ValueError):
        E.weld_mesh(torch.zeros(1, 3, 3))


@pytest.mark.parametrize("name", ["three_valued", "noise23"])
def test_two_runs_give_the_same_bits(name):
    tris = _case(name)[0]
    a = [t.clone() for t in E.weld_mesh(tris, normals=True)]
    b = E.weld_mesh(tris, normals=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_pipeline_keeps_the_mesh_on_the_device(tmp_path):
    """convert_to_explicit of one grid given as a GPU tensor and as a numpy array: the same mesh both ways and the same as the
    numpy weld of the host soup, down to the bytes of the OBJ; the mesh carries its GPU tensor, and the turntable renders from
    it - the same frames as from the host soup - without a host copy of the triangles ever being made."""
    opt = edict(dict(device="cuda", output_path=str(tmp_path), eval=dict(range=[-1.5, 1.5], num_points=100)))
    vol = _sphere(33, 0.8)[0]
    from_gpu, from_host = E.convert_to_explicit(opt, [torch.from_numpy(vol).cuda(), vol], isoval=0.5)
    assert isinstance(from_gpu.device_triangles, torch.Tensor) and from_gpu.device_triangles.is_cuda
    assert from_gpu._triangles is None and from_gpu._indexed is None             # nothing copied, nothing welded yet
    frames = V.visualize_mesh(from_gpu, str(tmp_path / "none"), resolution=(32, 32), write_gif=False, write_frames=False,
                              n_frames=9)      # (9 // 3 = 3 per full circle, 9 // 6 = 1 per half: 8 frames)
    assert from_gpu._triangles is None                                           # rendered from HBM
    empty = E.SimpleMesh(torch.zeros(0, 3, 3, device="cuda"))
    V.dump_meshes_viz(opt, ["e"], "mesh_viz", [empty], folder="viz")             # its length check reads the tensor's shape
    assert empty._triangles is None and not list((tmp_path / "viz").glob("*"))
    host = E.SimpleMesh(from_gpu.device_triangles.cpu().numpy())                 # the numpy path
    for other in (from_host, host):
        for attr in ("vertices", "faces", "triangles"):
            a, b = getattr(from_gpu, attr), getattr(other, attr)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), attr
    assert from_gpu.vertices.dtype == np.float32 and from_gpu.faces.dtype == np.int64 and from_gpu.triangles.dtype == np.float32
    assert np.array_equal(from_gpu.vertices.view(np.uint32), host.vertices.view(np.uint32))
    assert np.abs(from_gpu.vertex_normals - host.vertex_normals).max() <= NORMAL_ATOL
    V.dump_meshes(opt, ["gpu", "host", "numpy"], "mesh", [from_gpu, from_host, host], folder="dump")
    V.dump_meshes(opt, ["gpu", "numpy"], "mesh_n", [from_gpu, host], folder="dump", normals=True)
    obj = [(tmp_path / "dump" / ("%s_mesh.obj" % k)).read_bytes() for k in ("gpu", "host", "numpy")]
    assert obj[0] == obj[1] == obj[2] and obj[0].count(b"\nv ") == len(host.vertices)
    assert (tmp_path / "dump" / "gpu_mesh_n.obj").read_bytes().count(b"\nvn ") == len(host.vertices)
    want = V.visualize_mesh(host.triangles, str(tmp_path / "none"), resolution=(32, 32), write_gif=False, write_frames=False,
                            n_frames=9)
    assert frames.shape == (8, 32, 32, 3) and frames.dtype == np.uint8 and np.array_equal(frames, want)
    assert (frames != 255).any()
