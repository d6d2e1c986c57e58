"""No GPU: what the point-gradient tests on the GPU lean on.  The oracle's decoder (oracle/decoder_ref.py) differentiated in
its query points against the reference's own gradients (tests/golden/make_points_grad_golden.py), so that the GPU tests can
use it at other shapes; the mesh-vertex -> field-position mapping restated in numpy; the OBJ text of
dump_meshes(normals="field"); the parameter-freezing context manager of Implicit.field_gradient."""
import os

import numpy as np
import pytest
import torch

from oracle import decoder_ref as R
from tests import points_grad_cases as C
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.eval_3D import SimpleMesh, mesh_to_field_points_host
from zeroshape_amd.utils.options import EasyDict as edict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_grad_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def oracle_gradients(name, lat, sem, pts, cot, dtype=torch.float32):
    """(logits, d sum(cot * logit) / d points) of the oracle's decoder on the CPU in ``dtype`` (cot None: ones)."""
    from zeroshape_amd.model.shape.implicit import Implicit
    ctor = C.case(name)["ctor"]
    pos = Implicit(**ctor).pos_embed.detach().numpy()
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in C.state_dict(name, pos).items()}
    p = torch.from_numpy(np.asarray(pts)).to(dtype).requires_grad_(True)
    sem_t = None if sem is None else torch.from_numpy(sem).to(dtype)
    logit, _ = R.implicit_forward.__wrapped__(sd, torch.from_numpy(lat).to(dtype), p, num_heads=ctor["num_heads"],
                                              pos_perlayer=ctor["pos_perlayer"], latent_semantic=sem_t)
    w = torch.ones_like(logit) if cot is None else torch.from_numpy(cot).to(dtype)
    g, = torch.autograd.grad((logit * w).sum(), p)
    return logit.detach().numpy(), g.numpy()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_oracle_point_gradients_vs_reference_golden(name, golden):
    """fp32 and fp64, both cotangents: within FACTOR x the reference's own fp32-to-fp64 distance of the reference's fp64
    gradient (relative to its largest entry); the fp64 oracle far closer than that."""
    lat, sem, pts, cot = C.inputs(name)
    e_ref = float(golden[name + ".e_ref"][0])
    assert 1e-7 < e_ref < 1e-4 and golden[name + ".g_sum64"].dtype == np.float64
    for which, c in (("g_sum", None), ("g_cot", cot)):
        g64 = golden[name + "." + which + "64"]
        lg, g = oracle_gradients(name, lat, sem, pts, c)
        assert g.shape == (C.B, C.M, 3)
        err = C.rel_error(g, g64)
        print("%s %s: oracle fp32 error / e_ref = %.2f" % (name, which, err / e_ref))
        assert err <= C.FACTOR * e_ref
        np.testing.assert_allclose(lg, golden[name + ".logit32"], atol=1e-5, rtol=0)
        lg, g = oracle_gradients(name, lat, sem, pts, c, torch.float64)
        assert C.rel_error(g, g64) <= 1e-9
        np.testing.assert_allclose(lg, golden[name + ".logit64"], atol=1e-10, rtol=0)
    angle, left_out = C.normal_angles(oracle_gradients(name, lat, sem, pts, None)[1], golden[name + ".g_sum64"])
    assert left_out == 0.0 and angle <= C.FACTOR * float(golden[name + ".angle_deg"][0])


def test_golden_error_measures_are_those_of_its_arrays(golden):
    for name in C.CASES:
        assert C.rel_error(golden[name + ".g_sum32"], golden[name + ".g_sum64"]) == pytest.approx(float(golden[name + ".e_ref"][0]))
        assert C.normal_angles(golden[name + ".g_sum32"], golden[name + ".g_sum64"])[0] == \
            pytest.approx(float(golden[name + ".angle_deg"][0]))
        cot = C.inputs(name)[3]
        np.testing.assert_allclose(golden[name + ".g_cot64"], golden[name + ".g_sum64"] * cot[..., None], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("G", [2, 17, 129])
def test_vertex_to_field_position_mapping(G):
    """Marching cubes writes grid index u as v = min + u (max - min) / G; the grid is linspace(min, max, G): the mapping takes v
    back to sample u's position (fractional u too), to fp32 rounding; and it is the formula, in float64."""
    lo, hi = -1.5, 1.5
    u = np.concatenate([np.arange(G, dtype=np.float64), np.random.RandomState(G).uniform(0, G - 1, 50)])
    v = (np.float32(lo) + u * (hi - lo) / G).astype(np.float32)
    p = mesh_to_field_points_host(np.stack([v, v[::-1], v], axis=1), lo, G)
    assert p.dtype == np.float32 and p.shape == (len(u), 3)
    want = lo + u * (hi - lo) / (G - 1)
    # v carries half an ulp of at most 1.5, stretched by G / (G - 1) <= 2; the result's own rounding adds half an ulp
    tol = 2 ** -24 * 1.5 * (G / (G - 1.0)) + 2 ** -24 * 1.5
    assert np.abs(p[:, 0] - want).max() <= tol and np.abs(p[:, 1] - want[::-1]).max() <= tol
    assert p[0, 0] == np.float32(lo) and abs(float(p[G - 1, 0]) - hi) <= tol
    v64 = v.astype(np.float64)
    assert np.array_equal(p[:, 2], (lo + (v64 - lo) * G / (G - 1)).astype(np.float32))
    assert mesh_to_field_points_host(np.zeros((0, 3), np.float32), lo, G).shape == (0, 3)


class _Stub(object):
    """What dump_meshes reads of a mesh, preset on the host."""

    def __init__(self, vertices, faces, field_normals):
        self.vertices, self.faces, self.field_normals = vertices, faces, field_normals

    @property
    def vertex_normals(self):
        raise AssertionError("normals='field' must not read the area-weighted normals")


def _obj_today(mesh, normals):
    """dump_meshes' text for normals=False / True as it was before normals='field' existed, a line at a time."""
    verts, faces = mesh.vertices, mesh.faces + 1
    out = ["# zeroshape_amd mesh: %d vertices, %d faces\n" % (len(verts), len(faces))]
    out += ["v %.6f %.6f %.6f\n" % tuple(v) for v in verts.astype(np.float64)]
    if normals:
        out += ["vn %.6f %.6f %.6f\n" % tuple(v) for v in mesh.vertex_normals.astype(np.float64)]
        out += ["f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in faces]
    else:
        out += ["f %d %d %d\n" % tuple(t) for t in faces]
    return "".join(out)


def test_dump_meshes_field_normals_text(tmp_path):
    rs = np.random.RandomState(4)
    verts = rs.uniform(-1.5, 1.5, (7, 3)).astype(np.float32)
    faces = rs.randint(0, 7, (5, 3)).astype(np.int64)
    fn = rs.randn(7, 3)
    fn = (fn / np.linalg.norm(fn, axis=1, keepdims=True)).astype(np.float32)
    fn[2] = [0.0, -0.0, 1.0]
    opt = edict(output_path=str(tmp_path))
    stubs = [_Stub(verts, faces, fn), _Stub(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float32))]
    V.dump_meshes(opt, ["a", "b"], "mesh", stubs, folder="dump", normals="field")
    lines = (tmp_path / "dump" / "a_mesh.obj").read_text().splitlines()
    assert lines[0] == "# zeroshape_amd mesh: 7 vertices, 5 faces" and len(lines) == 1 + 7 + 7 + 5
    assert lines[1:8] == ["v %.6f %.6f %.6f" % tuple(v) for v in verts.astype(np.float64)]
    assert lines[8:15] == ["vn %.6f %.6f %.6f" % tuple(v) for v in fn.astype(np.float64)]
    assert lines[15:] == ["f %d//%d %d//%d %d//%d" % (a, a, b, b, c, c) for a, b, c in faces + 1]
    assert (tmp_path / "dump" / "b_mesh.obj").read_text() == "# zeroshape_amd mesh: 0 vertices, 0 faces\n"
    with pytest.raises(ValueError, match="'field'"):
        V.dump_meshes(opt, ["a"], "mesh", stubs[:1], folder="dump", normals="vertex")
    # a real mesh that never got field normals says what to call
    with pytest.raises(ValueError, match="eval_3D.field_normals"):
        V.dump_meshes(opt, ["c"], "mesh", [SimpleMesh(np.zeros((1, 3, 3), np.float32))], folder="dump", normals="field")


def test_dump_meshes_other_modes_keep_their_bytes(tmp_path):
    from oracle import mc_ref as M
    from tests.test_oracle_mc import _sphere
    tris = M.marching_cubes(_sphere(9, 0.8)[0], 0.5, np.float32(3.0 / 9), np.float32(-1.5))
    awkward = np.array([[[0.0, -0.0, 1e-7], [-1.5, 1234.5678, 0.1], [1e10, -2.5e-7, 0.3333333]]], np.float32)
    meshes = [SimpleMesh(tris), SimpleMesh(np.zeros((0, 3, 3), np.float32)), SimpleMesh(awkward)]
    assert len(meshes[0].vertices) > 10
    opt = edict(output_path=str(tmp_path))
    V.dump_meshes(opt, ["a", "b", "c"], "plain", meshes, folder="dump")
    V.dump_meshes(opt, ["a", "b", "c"], "vn", meshes, folder="dump", normals=True)
    for i, mesh in zip("abc", meshes):
        assert (tmp_path / "dump" / ("%s_plain.obj" % i)).read_bytes() == _obj_today(mesh, False).encode()
        assert (tmp_path / "dump" / ("%s_vn.obj" % i)).read_bytes() == _obj_today(mesh, True).encode()


def test_field_normals_refuses_host_meshes():
    from zeroshape_amd.utils import eval_3D as E
    opt = edict(eval=edict(vox_res=16, range=[-1.5, 1.5]))
    with pytest.raises(ValueError, match="host array"):
        E.field_normals(opt, None, torch.zeros(1, 197, 256), None, [SimpleMesh(np.zeros((1, 3, 3), np.float32))])


def test_frozen_parameters_restores_the_flags():
    from zeroshape_amd.model.shape.implicit import Implicit, frozen_parameters
    net = Implicit(**C.CASES["head"]["ctor"])
    net.norm.bias.requires_grad_(False)                    # a flag that was already off stays off
    before = {k: p.requires_grad for k, p in net.named_parameters()}
    ids = {k: id(p) for k, p in net.named_parameters()}
    assert not before["pos_embed"] and not before["norm.bias"] and before["norm.weight"]
    with frozen_parameters(net) as same:
        assert same is net and not any(p.requires_grad for p in net.parameters())
        assert {k: id(p) for k, p in net.named_parameters()} == ids          # the same objects: the operand cache's keys
    assert {k: p.requires_grad for k, p in net.named_parameters()} == before
    with pytest.raises(KeyError):
        with frozen_parameters(net):
            assert not net.norm.weight.requires_grad
            raise KeyError("inside")
    assert {k: p.requires_grad for k, p in net.named_parameters()} == before
    assert all(p.grad is None for p in net.parameters())
