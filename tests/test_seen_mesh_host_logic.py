"""CPU: the host half of the seen-surface meshes and point-cloud dumps - the numpy restatement of the kernel's rules plus
write_seen_surface_obj reproduce the files the reference's create_seen_surface wrote (tests/golden/seen_mesh_golden.npz), the
PLY writers round-trip, zs_seen_mesh checks its arguments before it touches the GPU, and evaluate() dumps only on request."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import seen_mesh_ref as R
from zeroshape_amd.utils import util_vis as V
from zeroshape_amd.utils.options import EasyDict as edict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seen_mesh_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_stored_inputs_keep_the_margins_the_construction_promises(golden):
    for case in R.STEPPED_CASES:
        m = R.assert_stepped_margins(golden[case + "_xyz"])
        print(case, m)
    assert R.margins(golden["s40x70_xyz"])["candidates"] == 2 * 39 * 69
    flat = R.margins(golden["flat12x12_xyz"])
    assert flat["emitted"] == flat["candidates"] == 2 * 11 * 11 and flat["edge_margin"] >= 0.05
    assert (golden["invalid5x6_xyz"][..., 2] <= -0.5).all()


@pytest.mark.parametrize("case", R.GOLDEN_CASES)
def test_restatement_and_writer_reproduce_the_reference_files(golden, case, tmp_path):
    xyz = golden[case + "_xyz"]
    H, W = xyz.shape[:2]
    verts, pixels, faces, vert_id = R.seen_mesh(xyz)
    assert verts.dtype == np.float32 and pixels.dtype == np.int32 and faces.dtype == np.int32
    assert (vert_id.ravel()[pixels] == np.arange(1, len(pixels) + 1)).all() and (vert_id > 0).sum() == len(pixels)
    V.write_seen_surface_obj(str(tmp_path), R.GOLDEN_SAMPLE_ID, R.GOLDEN_OBJ_NAME, R.GOLDEN_IMG, verts, pixels, faces, H, W)
    stem = os.path.join(str(tmp_path), "{}_{}".format(R.GOLDEN_SAMPLE_ID, R.GOLDEN_OBJ_NAME))
    for ext in ("obj", "mtl"):
        with open(stem + "." + ext, "rb") as f:
            assert f.read() == golden[case + "_" + ext].tobytes(), (case, ext)


def test_seen_surface_mesh_has_no_cpu_path():
    with pytest.raises(ValueError):
        V.seen_surface_mesh(torch.zeros(1, 4, 4, 3))
    with pytest.raises(ValueError):
        V.create_seen_surface("0", "0_image_input.png", torch.zeros(4, 4, 3), "/nonexistent", "seen_surface_fixed")


def read_ply(path):
    """Binary little-endian PLY -> (header lines, structured vertex array)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").split("\n")[:-1]
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0" and header[-1] == "end_header"
    elements = [h.split() for h in header if h.startswith("element")]
    assert len(elements) == 1 and elements[0][1] == "vertex"
    props = [h.split()[1:] for h in header if h.startswith("property")]
    assert props == [["float", "x"], ["float", "y"], ["float", "z"], ["uchar", "red"], ["uchar", "green"],
                     ["uchar", "blue"], ["uchar", "alpha"]]
    kinds = {"float": "<f4", "uchar": "u1"}
    data = np.frombuffer(raw[end:], np.dtype([(name, kinds[kind]) for kind, name in props]))
    assert len(data) == int(elements[0][2]) and len(raw) - end == 16 * len(data)
    return header, data


def _xyz(data):
    return np.stack([data["x"], data["y"], data["z"]], 1)


def test_pointcloud_writers_round_trip(tmp_path):
    opt = edict(output_path=str(tmp_path))
    rng = np.random.RandomState(0)
    preds = [torch.from_numpy(rng.randn(n, 3).astype(np.float32)) for n in (5, 0, 7)]
    gts = [torch.from_numpy(rng.randn(n, 3).astype(np.float32)) for n in (3, 4, 0)]
    V.dump_pointclouds_compare(opt, [10, 11, 12], "seen_surface", preds, gts, folder="dump")
    for i, pred, gt in zip((10, 11, 12), preds, gts):
        _, data = read_ply(tmp_path / "dump" / ("%d_seen_surface.ply" % i))
        n1, n2 = len(pred), len(gt)
        assert len(data) == n1 + n2
        assert _xyz(data).tobytes() == np.vstack([pred.numpy(), gt.numpy()]).tobytes()          # bit-equal
        rgb = np.stack([data["red"], data["green"], data["blue"]], 1)
        assert (rgb[:n1] == [255, 0, 0]).all() and (rgb[n1:] == [0, 255, 0]).all()            # red first, then green
        assert (data["alpha"] == 255).all()
    # colours given, and scalar colours through the jet table
    from zeroshape_amd.utils.eval_3D import _jet_lut
    pc = torch.from_numpy(rng.randn(6, 3).astype(np.float32))
    rgb = rng.randint(0, 256, size=(6, 3)).astype(np.uint8)
    scalar = np.array([[0.0], [0.25], [0.5], [0.75], [1.0], [0.1]], np.float32)
    V.dump_pointclouds(opt, ["a", "b"], "attn_pc", [pc, pc], [torch.from_numpy(rgb), torch.from_numpy(scalar)], folder="dump")
    _, a = read_ply(tmp_path / "dump" / "a_attn_pc.ply")
    _, b = read_ply(tmp_path / "dump" / "b_attn_pc.ply")
    assert _xyz(a).tobytes() == pc.numpy().tobytes() and (np.stack([a["red"], a["green"], a["blue"]], 1) == rgb).all()
    assert (np.stack([b["red"], b["green"], b["blue"]], 1) == _jet_lut()[np.uint8(255 * scalar[:, 0])]).all()
    assert (a["alpha"] == 255).all() and (b["alpha"] == 255).all()
    with pytest.raises(ValueError):
        V.dump_pointclouds(opt, ["c"], "attn_pc", [pc], [torch.from_numpy(scalar)], folder="dump", colormap="viridis")


def test_seen_mesh_arguments_are_checked_before_anything_is_touched():
    """0 + a message that starts with the entry point's name, or 1 for an empty problem, before any pointer is dereferenced or
    anything is launched (a 64-byte host buffer stands in for every non-null pointer)."""
    from zeroshape_amd import _lib, build
    build.build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(batch=2, H=9, W=13, thr=0.005, xyz=p, mask=None, vert_id=p, vert_pixel=p, verts=p, faces=p, counts=p, ws=p):
        return lib.zs_seen_mesh(xyz, mask, batch, H, W, thr, vert_id, vert_pixel, verts, faces, counts, ws, None)

    def fails(rc, what):
        assert rc == 0, what
        msg = lib.zs_last_error()
        assert msg.startswith(b"zs_seen_mesh: ") and what.encode() in msg, (what, msg)

    for kw in (dict(batch=-1), dict(H=-9), dict(W=-13)):
        fails(call(**kw), "negative")
    for name in ("xyz", "vert_id", "vert_pixel", "verts", "faces", "counts", "ws"):
        fails(call(**{name: None}), "null")
    for thr in (0.0, -0.005, float("nan"), float("inf")):
        fails(call(thr=thr), "bad threshold")
    assert call(batch=0) == 1 and call(H=0) == 1 and call(W=0) == 1
    assert call(batch=0, xyz=None, vert_id=None, counts=None, ws=None) == 1
    fails(call(batch=2 ** 20, H=2 ** 10, W=2), "too large")
    assert lib.zs_seen_mesh_workspace_bytes(2, 9, 13) == (2 * 2 + 1 + 1 + 1) * 8        # 2 x 2 units + 1 | 1 tile + 1
    assert lib.zs_seen_mesh_workspace_bytes(28, 224, 224) == (28 * 784 + 1 + 11 + 1) * 8
    assert lib.zs_seen_mesh_workspace_bytes(0, 9, 13) == 0 and lib.zs_seen_mesh_workspace_bytes(1, -1, 4) == 0


@pytest.mark.parametrize("task", ["shape", "depth"])
def test_dump_switch_is_a_command_line_option_the_yaml_files_do_not_carry(task, tmp_path):
    from zeroshape_amd.utils import options
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["--yaml=%s/options/%s.yaml" % (root, task), "--output_root=%s" % tmp_path]
    assert "dump_results" not in options.load_options(base[0][len("--yaml="):]).eval
    assert "dump_results" not in options.set(options.parse_arguments(base), need_gpu=False).eval
    assert options.set(options.parse_arguments(base + ["--eval.dump_results"]), need_gpu=False).eval.dump_results is True
    with pytest.raises(KeyError):                     # the fence around unknown keys stands
        options.set(options.parse_arguments(base + ["--eval.dump_result"]), need_gpu=False)


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, opt, var, ep, write_new=False, train=False):
        self.calls.append((list(torch.as_tensor(var.idx).view(-1).tolist()), write_new))


def _batches():
    return [dict(idx=torch.tensor([0, 1]), category_label=torch.tensor([0, 0])),
            dict(idx=torch.tensor([2]), category_label=torch.tensor([0]))]


def _runner(cls, rec):
    r = object.__new__(cls)
    r.reducer = None
    r.graph = types.SimpleNamespace(eval=lambda: None, impl_network=None)
    r.test_loader, r.test_data = _batches(), range(3)
    r.evaluate_batch = lambda opt, var, ep=None, it=None, single_gpu=False: var
    r.dump_results = rec
    return r


@pytest.mark.parametrize("engine", ["shape", "depth"])
def test_evaluate_dumps_results_only_on_request(engine, monkeypatch):
    """Runner.evaluate(training=False) calls dump_results once per batch when opt.eval.dump_results is set (the first call
    with write_new), and not at all when the key is absent, false, or the evaluation is a validation pass of training."""
    if engine == "shape":
        from zeroshape_amd.model import shape_engine as E

        def eval_metrics(opt, var, net):
            n = len(var.idx)
            var.cd_acc, var.cd_comp, var.f_score = torch.ones(n), torch.ones(n), torch.ones(n, 2)
        monkeypatch.setattr(E.eval_3D, "eval_metrics", eval_metrics)
    else:
        from zeroshape_amd.model import depth_engine as E
        monkeypatch.setattr(E.util, "print_eval", lambda *a, **k: None)
    for flag, training, expected in ((None, False, []), (False, False, []), (True, True, []),
                                     (True, False, [([0, 1], True), ([2], False)])):
        rec = _Recorder()
        r = _runner(E.Runner, rec)
        if engine == "depth":
            r.depth_metric = types.SimpleNamespace(
                metric_keys=["rmse", "l1_err"],
                compute_metrics=lambda pred, gt, mask: ({k: torch.ones(len(pred)) for k in ("rmse", "l1_err")}, pred))
            for b in r.test_loader:
                b.update(depth_pred=torch.zeros(len(b["idx"]), 1, 2, 2), depth_input_map=torch.zeros(len(b["idx"]), 1, 2, 2),
                         mask_input_map=torch.ones(len(b["idx"]), 1, 2, 2))
        opt = edict(device="cpu", output_path=None, eval=dict(f_thresholds=[0.01, 0.02]), data=dict(dataset_test="synthetic"))
        if flag is not None:
            opt.eval.dump_results = flag
        r.evaluate(opt, ep=0, training=training)
        assert rec.calls == expected, (engine, flag, training)
