"""The C-ABI library loads on a GPU-less host and exports exactly what include/zeroshape_hip.h
declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "zeroshape_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(zs_\w+)\s*\(", txt)))


@pytest.fixture(scope="module")
def lib():
    from zeroshape_amd import build, _lib
    build.build()
    return _lib.load()


def test_header_and_binding_agree(lib):
    from zeroshape_amd import _lib
    names = _declared()
    assert len(names) >= 9
    assert sorted(_lib.SIGNATURES) == names


def test_every_declared_symbol_is_exported(lib):
    from zeroshape_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert getattr(raw, name) is not None


def test_versions_and_sizes(lib):
    from zeroshape_amd import program as P
    hdr = open(os.path.join(ROOT, "include", "zeroshape_hip.h")).read()
    assert lib.zs_abi_version() == int(re.search(r"#define ZS_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.zs_sdf_program_bytes() == P.PROGRAM_BYTES
    assert lib.zs_sdf_prologue_scratch_bytes() == P.SCRATCH_FLOATS * 4
    assert lib.zs_sdf_workspace_bytes() == 256 * 4 * 3 * 32768 + 4096
    assert lib.zs_sdf_attn_scratch_bytes(2, 129) == 2 * 2 * 4 * (16 * 7 * 4 * 64 * 16 + 16 * 9 * 64 * 4)
    assert lib.zs_sdf_attn_scratch_bytes(0, 5) == 0
    assert lib.zs_last_error() in (b"", None) or isinstance(lib.zs_last_error(), bytes)


def test_retired_evaluation_geometry_symbols_are_gone(lib):
    """ABI 46 removed the pose search's unsorted entry and its scratch size, the uniform-grid arm and the Z-order sort:
    none of them is named in the header (comments included), bound in SIGNATURES or exported by the built library, and
    the library no longer carries the kernels that only they launched."""
    from zeroshape_amd import _lib
    removed = ["zs_pose_search_batch", "zs_pose_search_batch_grid", "zs_pose_gt_grid", "zs_pose_grid_bytes",
               "zs_morton_sort", "zs_morton_scratch_bytes", "zs_pose_scratch_bytes"]
    kernels = [b"pose_gt_grid_kernel", b"pose_pred_grid_kernel", b"pose_nn_grid_kernel", b"morton_key_kernel",
               b"morton_gather_kernel", b"14nn_both_kernel"]        # (the last: its mangled name, length prefix included)
    hdr = open(os.path.join(ROOT, "include", "zeroshape_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in removed:
        assert not re.search(r"\b%s\b" % name, hdr), name
        assert name not in _lib.SIGNATURES, name
        assert not hasattr(raw, name), name
    for name in kernels:
        assert name not in blob, name
    assert b"pose_nn_soa_kernel" in blob and b"nn_both_sgpr_kernel" in blob      # (the probe does see kernel names)
    assert lib.zs_abi_version() == 46


def test_pose_search_selector_is_checked_before_any_device_work():
    """brute_force_search takes nn = "cull", "pairs" or "brute"; anything else - the retired "grid" included - raises
    ValueError naming the three before a tensor is moved or the library is loaded (so it does here, without a GPU)."""
    import torch
    from zeroshape_amd.utils import eval_3D as E
    for bad in ("grid", "nonsense", "CULL", ""):
        with pytest.raises(ValueError, match="'cull', 'pairs' or 'brute'"):
            E.brute_force_search(torch.zeros(5, 3), torch.zeros(3, 3), device="cuda", nn=bad)


def test_python_constants_equal_the_header():
    """Every #define ZS_ACT_* / ZS_CONV_* has a Python constant of the same value in nn/ops.py (the one place in nn/ that
    writes them), and the names nn/autograd.py and nn/operands.py hand on are those objects' values."""
    from zeroshape_amd.nn import autograd as A, operands, ops
    hdr = open(os.path.join(ROOT, "include", "zeroshape_hip.h")).read()
    defines = {name: int(value, 0) for name, value in re.findall(r"^#define ZS_((?:ACT|CONV)_\w+)[ \t]+(\w+)", hdr, flags=re.M)}
    assert sum(n.startswith("ACT_") for n in defines) >= 5 and sum(n.startswith("CONV_") for n in defines) >= 13
    for name, value in defines.items():
        assert getattr(ops, name) == value, name
    python = {n for n in vars(ops) if re.fullmatch(r"(ACT|CONV)_[A-Z0-9_]+", n) and isinstance(getattr(ops, n), int)}
    assert python == set(defines)
    for mod in (A, operands):
        for name in defines:
            if hasattr(mod, name):
                assert getattr(mod, name) == defines[name], (mod.__name__, name)
    assert all(hasattr(A, n) for n in defines if n.startswith("ACT_"))


def test_argument_errors_are_reported_without_touching_the_gpu(lib):
    from zeroshape_amd import _lib
    # the retired convolution flag bits (64, 256: the removed stream-K kernels) fail loudly at all three entry points
    conv = [None] * 7 + [1, 8, 8, 16, 8, 8, 16, 1, 1, 1, 0, 0]
    for bit in (64, 256):
        assert lib.zs_conv2d_nhwc(*conv, 16 | bit, 1.0, 0.0, 0, None) == 0 and b"retired" in lib.zs_last_error()
        assert lib.zs_conv2d_nhwc_ws(*conv, 16 | bit, 1.0, 0.0, 0, None, None) == 0 and b"retired" in lib.zs_last_error()
        assert lib.zs_conv2d_nhwc_fused(*conv, 16 | 128 | bit, 1.0, 0.0, 0, ctypes.byref(_lib.ConvFuse()), None, None) == 0
        assert b"retired" in lib.zs_last_error()
    # negative sizes / null pointers are rejected before any HIP call: 0 + message
    assert lib.zs_chamfer_forward(None, None, 1, -1, 3, None, None, None, None, None) == 0
    assert b"negative" in lib.zs_last_error()
    assert lib.zs_chamfer_forward(None, None, 1, 4, 3, None, None, None, None, None) == 0
    assert b"null" in lib.zs_last_error()
    assert lib.zs_sdf_query_grid(None, 0, 1, None, 9, 3, 2, 1, None, None, None, None) == 0
    assert b"bad range" in lib.zs_last_error()
    # empty problems succeed trivially (nothing to launch)
    assert lib.zs_chamfer_forward(None, None, 0, 4, 3, None, None, None, None, None) == 1
    assert lib.zs_sdf_query_points(None, 0, 0, None, 5, None, None, None, None, None) == 1


def test_decoder_query_arguments_are_checked_before_anything_is_touched(lib):
    """All six zs_sdf_query_* entry points, both arithmetics: 0 + a message that starts with the called entry point's own
    name, or 1 for an empty problem - before any pointer is dereferenced or anything is launched (a 64-byte host buffer
    stands in for every non-null pointer)."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    pb = lib.zs_sdf_program_bytes()

    def fails(name, call, what):
        assert call == 0, (name, what)
        msg = lib.zs_last_error()
        assert msg.startswith(name.encode() + b": ") and what.encode() in msg, (name, what, msg)

    for name in ("zs_sdf_query_points", "zs_sdf_query_points_split"):
        fn = getattr(lib, name)
        opt = (None,) if name == "zs_sdf_query_points" else ()        # (the attention map of the fp32 form)

        def points(prog, stride, batch, m, data):
            return fn(prog, stride, batch, data, m, data, *opt, None, data, None)

        fails(name, points(p, pb, -1, 5, p), "negative size")
        fails(name, points(p, pb, 2, -5, p), "negative size")
        assert points(None, 0, 0, 5, None) == 1 and points(None, 0, 2, 0, None) == 1
        fails(name, points(p, pb, 2, 300, None), "null pointer")
        fails(name, points(None, pb, 2, 300, p), "null pointer")
        fails(name, points(p, pb + 8, 2, 300, p), "bad program stride")
        fails(name, points(p, pb - 16, 2, 300, p), "bad program stride")
        fails(name, points(p, pb, 200, 2 ** 31 - 1, p), "too many tiles")

    # G = 9: slices of 81 points, 729 points
    forms = [("zs_sdf_query_grid", 9, 10, "split the slab", 2048), ("zs_sdf_query_grid_split", 9, 10, "split the slab", 2048),
             ("zs_sdf_query_grid_range", 729, 730, "split the range", 2048 ** 3),
             ("zs_sdf_query_grid_range_split", 729, 730, "split the range", 2048 ** 3)]
    for name, whole, past, hint, whole_2048 in forms:
        fn = getattr(lib, name)

        def grid(prog, stride, batch, G, begin, end, data):
            return fn(prog, stride, batch, data, G, begin, end, 1, data, None, data, None)

        fails(name, grid(p, pb, -1, 9, 0, whole, p), "bad range")
        fails(name, grid(p, pb, 2, 0, 0, 0, p), "bad range")
        fails(name, grid(p, pb, 2, 9, 3, 2, p), "bad range")
        fails(name, grid(p, pb, 2, 9, 0, past, p), "bad range")
        fails(name, grid(p, pb, 2, 9, -1, whole, p), "bad range")
        assert grid(None, 0, 0, 9, 0, whole, None) == 1 and grid(None, 0, 2, 9, 4, 4, None) == 1
        fails(name, grid(p, pb, 2, 9, 0, whole, None), "null pointer")
        fails(name, grid(None, pb, 2, 9, 0, whole, p), "null pointer")
        fails(name, grid(p, pb + 8, 2, 9, 0, whole, p), "bad program stride")
        fails(name, grid(p, pb - 16, 2, 9, 0, whole, p), "bad program stride")
        fails(name, grid(p, pb, 1, 2048, 0, whole_2048, p), "exceed 2^31")
        assert hint.encode() in lib.zs_last_error()


def test_product_path_fails_loudly_without_library(monkeypatch):
    from zeroshape_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libzeroshape_hip.so")
    with pytest.raises(_lib.ZeroShapeHipError):
        _lib.load()


def test_cpu_tensors_are_rejected_not_emulated():
    import torch
    from zeroshape_amd import chamfer_3D
    x = torch.rand(1, 4, 3)
    d = torch.zeros(1, 4)
    i = torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(ValueError):
        chamfer_3D.forward(x, x, d, d, i, i)
    from zeroshape_amd.model.shape.implicit import Implicit
    m = Implicit(196, latent_dim=256, n_channels=256, n_blocks_attn=2, n_layers_mlp=8, num_heads=8,
                 skip_in=[2, 4, 6], pos_perlayer=False).eval()
    with pytest.raises(ValueError):
        m(torch.zeros(1, 197, 256), None, torch.zeros(1, 4, 3))
