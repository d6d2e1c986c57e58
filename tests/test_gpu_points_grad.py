"""GPU: `Implicit` differentiated in its query points (zs_posenc3d_bwd + the data gradients training already had, nn/autograd.py),
Implicit.field_gradient, and the field's normals on marching-cubes meshes (csrc/field_normals.hip, eval_3D.field_normals,
dump_meshes(normals="field")) - against the reference's own gradients (tests/golden/make_points_grad_golden.py) and, at other
shapes, the oracle's autograd on the CPU (held to the same file by tests/test_points_grad_host_logic.py).

The bound on a gradient: FACTOR = 8 x e_ref of the configuration - the reference's own fp32-to-fp64 distance, read from the
fixture - relative to max|g64|.  On angles: 8 x the fixture's largest fp32-to-fp64 angle, vertices with |g64| below 1e-3 x the
median left out, at most 1 % of them.  The measured ratios are recorded in profiles/points_grad_checks.md."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import points_grad_cases as C
from tests.test_points_grad_host_logic import oracle_gradients
from zeroshape_amd import synthetic as syn

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_grad_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _build(ctor, sd_cfg, seed):
    from zeroshape_amd.model.shape.implicit import Implicit
    m = Implicit(**ctor)
    sd = syn.seeded_state_dict(seed=seed, pos_embed=m.pos_embed.detach().numpy(), **sd_cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda().eval()


_NETS = {}


def _net(name):
    if name not in _NETS:
        case = C.case(name)
        _NETS[name] = _build(case["ctor"], case["syn"], case["seed"])
    return _NETS[name]


def _cuda(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _no_grads(net):
    for p in net.parameters():
        p.grad = None


# ---- 1, 2: the gradient of forward() against the reference's, and the logits it comes with ----
@pytest.mark.parametrize("which", ["g_sum", "g_cot"])
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_point_gradient_vs_reference_golden(name, which, golden):
    net = _net(name)
    lat, sem, pts, cot = _cuda(*C.inputs(name))
    pts.requires_grad_()
    logits = net(lat, sem, pts)[0]
    assert logits.requires_grad
    (logits.sum() if which == "g_sum" else (logits * cot).sum()).backward()
    assert pts.grad is not None and pts.grad.shape == (C.B, C.M, 3) and bool(torch.isfinite(pts.grad).all())
    e_ref, g64 = float(golden[name + ".e_ref"][0]), golden[name + "." + which + "64"]
    err = C.rel_error(pts.grad.cpu().numpy(), g64)
    print("%s %s: GPU error / e_ref = %.2f (e_ref %.2e)" % (name, which, err / e_ref, e_ref))
    assert err <= C.FACTOR * e_ref
    np.testing.assert_allclose(logits.detach().cpu().numpy(), golden[name + ".logit64"], atol=2e-5, rtol=0)
    _no_grads(net)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_logits_are_those_of_the_latent_gradient_route(name):
    """Bit for bit the logits of the call the layer-by-layer path served before: the latent requires a gradient, the points do
    not.  Asking for the point gradient changes no forward launch."""
    net = _net(name)
    lat, sem, pts, _ = _cuda(*C.inputs(name))
    a = net(lat, sem, pts.clone().requires_grad_(), need_attn=False)[0]
    b = net(lat.clone().requires_grad_(), sem, pts, need_attn=False)[0]
    assert a.requires_grad and b.requires_grad and torch.equal(a.detach(), b.detach())
    with torch.no_grad():                       # ... and grad mode off still takes the inference route, whatever the points' flag
        c = net(lat, sem, pts.clone().requires_grad_(), need_attn=False)[0]
    assert not c.requires_grad


def test_second_order_request_fails_loudly():
    for name in ("yaml", "posenc4"):
        net = _net(name)
        lat, sem, pts, _ = _cuda(*C.inputs(name, batch=1, m=5))
        pts.requires_grad_()
        logits = net(lat, sem, pts, need_attn=False)[0]
        with pytest.raises(RuntimeError, match="first-order"):
            torch.autograd.grad(logits.sum(), pts, create_graph=True)
        _no_grads(net)


# ---- 3: edge shapes against the oracle's autograd ----
@pytest.mark.parametrize("L", [0, 1, 4])
@pytest.mark.parametrize("B,M", [(1, 1), (1, 63), (3, 65), (2, 257)])
def test_point_gradient_edge_shapes_vs_oracle(B, M, L, golden):
    """A single row, both sides of the 64-row tile, several tiles; 3, 9 (padded to 12) and 27 (padded to 28) point channels.
    The unit of the bound is the fixture's: e_ref of the yaml configuration for L = 0, of posenc4 for L = 4, and for L = 1, which
    the fixture does not hold, the smaller of the two."""
    name = {0: "yaml", 1: "posenc1", 4: "posenc4"}[L]
    net = _net(name)
    lat, sem, pts, _ = C.inputs(name, batch=B, m=M)
    _, g64 = oracle_gradients(name, lat, sem, pts, None, torch.float64)
    e_ref = {0: float(golden["yaml.e_ref"][0]), 4: float(golden["posenc4.e_ref"][0])}
    e_ref[1] = min(e_ref.values())
    lat_d, pts_d = _cuda(lat, pts)
    pts_d.requires_grad_()
    net(lat_d, None, pts_d, need_attn=False)[0].sum().backward()
    err = C.rel_error(pts_d.grad.cpu().numpy(), g64)
    print("B %d M %d L %d: GPU error / e_ref = %.2f" % (B, M, L, err / e_ref[L]))
    assert pts_d.grad.shape == (B, M, 3) and err <= C.FACTOR * e_ref[L]
    _no_grads(net)


# ---- 4: the encoding's adjoint alone ----
@pytest.mark.parametrize("L", [1, 4, 10])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_posenc3d_bwd_vs_torch_autograd(n, L):
    """Against torch's autograd of the oracle's encoding in float64.  x 2^k is exact in fp32, so both sides take sin / cos of the
    same angles; what differs is sinf / cosf (a few ulp of 1) and the rounding of ~4 L products and sums, each relative 2^-24:
    per entry well inside 2^-21 x (|denc_x| + sum_k 2^k (|denc_sin_k| + |denc_cos_k|)).  The cotangent's padding channels are
    NaN: a kernel that read them could not return finite numbers."""
    from oracle import decoder_ref as R
    from zeroshape_amd.nn import autograd as A, ops
    rs = np.random.RandomState(100 * n + L)
    x = rs.uniform(-0.6, 0.6, (n, 3)).astype(np.float32)
    E, stride = 3 + 6 * L, (3 + 6 * L + 3) // 4 * 4
    assert stride > E
    denc = np.full((n, stride), np.nan, np.float32)
    denc[:, :E] = rs.randn(n, E)
    xr = torch.from_numpy(x).double().requires_grad_(True)
    (R.posenc_3d(xr, L).double() * torch.from_numpy(denc[:, :E]).double()).sum().backward()
    got = ops.posenc3d_bwd(torch.from_numpy(x).cuda(), L, torch.from_numpy(denc).cuda()).cpu().numpy()
    assert got.shape == (n, 3) and np.isfinite(got).all()
    mag = np.abs(denc[:, :3]).astype(np.float64)
    for k in range(L):
        mag += 2.0 ** k * (np.abs(denc[:, 3 + 6 * k:6 + 6 * k]) + np.abs(denc[:, 6 + 6 * k:9 + 6 * k]))
    assert (np.abs(got - xr.grad.numpy()) <= 2.0 ** -21 * mag).all()
    # the Function over it: the same numbers through autograd, and no graph at all for points without a gradient
    xg = torch.from_numpy(x).cuda().requires_grad_()
    enc = A.posenc3d(xg, L)
    enc.backward(torch.from_numpy(denc).cuda())
    assert np.array_equal(xg.grad.cpu().numpy(), got)
    plain = A.posenc3d(torch.from_numpy(x).cuda(), L)
    assert not plain.requires_grad and plain.grad_fn is None and torch.equal(plain, enc.detach())


# ---- 5: training does not notice ----
def test_parameter_gradients_do_not_depend_on_the_points_flag():
    net = _net("yaml")
    lat, _, pts, cot = _cuda(*C.inputs("yaml", batch=2, m=65))
    keep = 0.9
    scales = [torch.tensor(v, dtype=torch.float32).cuda() / keep for v in ([1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 1.0])]
    grads = []
    try:
        net.train()
        net.drop_scales = scales
        for flag in (False, True):
            _no_grads(net)
            p = pts.clone().requires_grad_(flag)
            (net(lat, None, p, need_attn=False)[0] * cot).sum().backward()
            assert (p.grad is not None) == flag
            grads.append({k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None})
    finally:
        net.eval()
        net.drop_scales = None
        _no_grads(net)
    assert len(grads[0]) > 20 and grads[0].keys() == grads[1].keys()
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


# ---- 6: field_gradient ----
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_field_gradient(name, golden):
    from zeroshape_amd.nn import autograd as A
    from zeroshape_amd.nn.operands import CACHE
    net = _net(name)
    lat, sem, pts, _ = _cuda(*C.inputs(name))
    e_ref, g64 = float(golden[name + ".e_ref"][0]), golden[name + ".g_sum64"]
    net.norm.bias.requires_grad_(False)
    try:
        _no_grads(net)
        flags = {k: p.requires_grad for k, p in net.named_parameters()}
        state = (A.SCRATCH_GENERATION[0], CACHE.epoch, len(CACHE.packs), A.CACHE is CACHE)
        with torch.no_grad():                                   # (it enables what it needs itself)
            logits, g_one = net.field_gradient(lat, sem, pts)
        logits64, g_chunks = net.field_gradient(lat, sem, pts, chunk=64)
        assert (A.SCRATCH_GENERATION[0], CACHE.epoch, len(CACHE.packs), A.CACHE is CACHE) == state and state[3]
        assert {k: p.requires_grad for k, p in net.named_parameters()} == flags
        assert all(p.grad is None for p in net.parameters())
    finally:
        net.norm.bias.requires_grad_(True)
    assert g_one.shape == (C.B, C.M, 3) and logits.shape == (C.B, C.M) and not g_one.requires_grad and not logits.requires_grad
    err_one, err_chunks = C.rel_error(g_one.cpu().numpy(), g64), C.rel_error(g_chunks.cpu().numpy(), g64)
    between = float((g_one - g_chunks).abs().max()) / np.abs(g64).max()
    print("%s: field_gradient error / e_ref = %.2f (one chunk), %.2f (chunks of 64); between the two %.2f"
          % (name, err_one / e_ref, err_chunks / e_ref, between / e_ref))
    assert err_one <= C.FACTOR * e_ref and err_chunks <= C.FACTOR * e_ref and between <= C.FACTOR * e_ref
    np.testing.assert_allclose(logits.cpu().numpy(), golden[name + ".logit64"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(logits64.cpu().numpy(), golden[name + ".logit64"], atol=2e-5, rtol=0)
    # the gradient forward() gives for a cotangent of ones is the same thing
    p = pts.clone().requires_grad_()
    net(lat, sem, p, need_attn=False)[0].sum().backward()
    assert float((p.grad - g_one).abs().max()) / np.abs(g64).max() <= C.FACTOR * e_ref
    _no_grads(net)
    empty = net.field_gradient(lat, sem, pts[:, :0])
    assert empty[0].shape == (C.B, 0) and empty[1].shape == (C.B, 0, 3)


def test_field_gradient_restores_the_flags_when_it_raises():
    net = _net("yaml")
    lat, _, pts, _ = _cuda(*C.inputs("yaml", batch=1, m=4))
    flags = [p.requires_grad for p in net.parameters()]
    with pytest.raises(ValueError):
        net.field_gradient(lat[:, :100], None, pts)                 # a latent of the wrong shape: raised inside the frozen block
    assert [p.requires_grad for p in net.parameters()] == flags and not net.training


# ---- 7, 8: normals on a mesh ----
def _opt(tmp=None):
    from zeroshape_amd.utils.options import EasyDict as edict
    return edict(dict(device="cuda", H=224, W=224, output_path=str(tmp), eval=dict(vox_res=16, range=[-1.5, 1.5]),
                      arch=dict(win_size=16)))


@pytest.fixture(scope="module")
def vox16():
    """(opt, latent [1,197,256] on the GPU, the vox-16 mesh of the yaml configuration's first image with its field normals)."""
    from zeroshape_amd.utils import eval_3D as E
    from zeroshape_amd.utils.options import EasyDict as edict
    opt, net = _opt(), _net("yaml")
    lat = _cuda(C.inputs("yaml")[0][:1])[0]
    grid = E.get_dense_3D_grid(opt, edict(dict(idx=[0])))
    occ, _ = E.compute_level_grid(opt, net, lat, None, grid, None)
    meshes = E.convert_to_explicit(opt, list(occ), isoval=0.5)
    assert E.field_normals(opt, net, lat, None, meshes, chunk=200) is meshes
    return opt, lat, meshes[0]


def test_field_normals_vs_oracle(vox16, golden):
    from zeroshape_amd import _lib
    from zeroshape_amd.utils import eval_3D as E
    opt, lat, mesh = vox16
    V = len(mesh.vertices)
    assert V > 100 and mesh.device_field_normals.is_cuda and mesh.device_field_normals.shape == (V, 3)
    n = mesh.field_normals
    assert n.dtype == np.float32 and n.shape == (V, 3) and mesh.field_normals is n
    assert int(mesh.field_normal_fallbacks.item()) == 0
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() <= 2 ** -23          # fp64 normalised, rounded once
    # the device mapping is the numpy restatement, bit for bit
    lib, dv = _lib.load(), torch.from_numpy(mesh.vertices).cuda()
    mapped = torch.empty_like(dv)
    _lib.check(lib.zs_mesh_to_field_points(_lib.ptr(dv), V, -1.5, 17, _lib.ptr(mapped), _lib.current_stream_ptr(dv.device)),
               "zs_mesh_to_field_points")
    host = E.mesh_to_field_points_host(mesh.vertices, -1.5, 17)
    assert np.array_equal(mapped.cpu().numpy(), host)
    _, g64 = oracle_gradients("yaml", lat.cpu().numpy(), None, host[None], None, torch.float64)
    angle, left_out = C.normal_angles(-n.astype(np.float64), g64[0])        # (normal_angles compares gradient directions)
    unit = float(golden["yaml.angle_deg"][0])
    print("vox-16 field normals: %d vertices, largest angle %.5f deg = %.2f x the fixture's %.5f; left out %.4f"
          % (V, angle, angle / unit, unit, left_out))
    assert left_out <= C.SKIP_MOST and angle <= C.FACTOR * unit
    # they point out of the surface: along the area-weighted normals of the mesh itself, on the whole
    assert ((n * mesh.vertex_normals).sum(1) > 0).mean() > 0.95


def test_field_normals_of_an_empty_mesh_and_the_fallback_rows(vox16):
    from zeroshape_amd import _lib
    from zeroshape_amd.utils import eval_3D as E
    opt, lat, _ = vox16
    meshes = E.convert_to_explicit(opt, [torch.zeros(17, 17, 17, device="cuda")], isoval=0.5)
    E.field_normals(opt, _net("yaml"), lat, None, meshes)
    assert meshes[0].field_normals.shape == (0, 3) and meshes[0].field_normals.dtype == np.float32
    assert int(meshes[0].field_normal_fallbacks.item()) == 0
    with pytest.raises(ValueError, match="host array"):
        E.field_normals(opt, _net("yaml"), lat, None, [E.SimpleMesh(np.zeros((1, 3, 3), np.float32))])
    lib = _lib.load()
    grad = torch.tensor([[0.0, 0.0, 0.0], [3.0, 0.0, -4.0], [float("nan"), 1.0, 0.0], [float("inf"), 0.0, 0.0]]).cuda()
    fallback = torch.tensor([[0.0, 1.0, 0.0], [9.0, 9.0, 9.0], [0.6, 0.0, 0.8], [1.0, 0.0, 0.0]]).cuda()
    for fb, want in ((fallback, [[0, 1, 0], [-0.6, 0, 0.8], [0.6, 0, 0.8], [1, 0, 0]]),
                     (None, [[0, 0, 0], [-0.6, 0, 0.8], [0, 0, 0], [0, 0, 0]])):
        out, count = torch.full((4, 3), 7.0).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
        _lib.check(lib.zs_field_normals_finish(_lib.ptr(grad), _lib.ptr(fb), 4, _lib.ptr(out), _lib.ptr(count),
                                               _lib.current_stream_ptr(grad.device)), "zs_field_normals_finish")
        assert int(count.item()) == 3
        assert np.array_equal(out.cpu().numpy(), np.array(want, np.float64).astype(np.float32))
    # one zero and one NaN row: the fallback rows and a count of 2
    out, count = torch.empty(2, 3).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    g2, f2 = grad[[0, 2]].contiguous(), fallback[[0, 2]].contiguous()       # (named: both alive while the kernel reads them)
    _lib.check(lib.zs_field_normals_finish(_lib.ptr(g2), _lib.ptr(f2), 2, _lib.ptr(out), _lib.ptr(count),
                                           _lib.current_stream_ptr(grad.device)), "zs_field_normals_finish")
    assert int(count.item()) == 2 and torch.equal(out, f2)
    assert lib.zs_mesh_to_field_points(_lib.ptr(grad), 4, -1.5, 1, _lib.ptr(out), None) == 0
    assert b"zs_mesh_to_field_points: bad grid" in lib.zs_last_error()


def test_obj_file_with_field_normals(vox16, tmp_path):
    from zeroshape_amd.utils import util_vis
    opt, _, mesh = vox16
    opt = _opt(tmp_path)
    util_vis.dump_meshes(opt, ["x"], "mesh", [mesh], folder="dump", normals="field")
    lines = (tmp_path / "dump" / "x_mesh.obj").read_text().splitlines()
    V, F = len(mesh.vertices), len(mesh.faces)
    v = [ln for ln in lines if ln.startswith("v ")]
    vn = [ln for ln in lines if ln.startswith("vn ")]
    f = [ln for ln in lines if ln.startswith("f ")]
    assert (len(v), len(vn), len(f), len(lines)) == (V, V, F, 1 + 2 * V + F)
    for ln, face in zip(f, mesh.faces + 1):
        assert ln.split()[1:] == ["%d//%d" % (a, a) for a in face]
    parsed = np.array([[float(t) for t in ln.split()[1:]] for ln in vn])
    assert np.abs(parsed - mesh.field_normals.astype(np.float64)).max() <= 0.5e-6 + 1e-12
    parsed_v = np.array([[float(t) for t in ln.split()[1:]] for ln in v])
    assert np.abs(parsed_v - mesh.vertices.astype(np.float64)).max() <= 0.5e-6 + 1e-12
