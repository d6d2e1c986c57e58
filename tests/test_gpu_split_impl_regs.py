"""impl_mlp in registers (csrc/sdf_decoder_split.hip: IMPL_MLP IN REGISTERS): the odd layers of impl_mlp take their B operands
from a second register array instead of the wave's LDS slab.  Every accumulator sees the same operands in the same order, so
the library is held to BIT equality with the slab form of the same source (-DZS_SPLIT_IMPL_SLAB, built beside it once per
session), under both block-0 arms; two identical launches stay bit-equal (a read too close behind an asm MFMA shows up as
run-to-run noise), and the point lists stay within 2.1e-6 of the exact-fp32 kernel, the figure DESIGN 3b.3 records
for them."""
import ctypes
import os
import subprocess

import pytest
import torch

from zeroshape_amd import _lib
from zeroshape_amd import build as B
from zeroshape_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_ATOL = 2.1e-6   # point lists, split arithmetic vs the exact-fp32 kernel
ARMS = (("stream", {}), ("gemm", {"ZS_SPLIT_BLOCK0_GEMM": "1"}))
SRC = "sdf_decoder_split.hip"


def build_slab_lib():
    """The library with the slab form of impl_mlp (tools/build_variant_lib.py's recipe, stamped like build.py's objects: it is
    rebuilt only when the source, its headers or the flags change)."""
    flags = B.COMMON + B.EXTRA[SRC] + ["-DZS_SPLIT_IMPL_SLAB"]
    out_dir = os.path.join(ROOT, "tools", "_timing")
    lib, stamp_file = os.path.join(out_dir, "impl_slab.so"), os.path.join(out_dir, "impl_slab.so.stamp")
    stamp = B._stamp(os.path.join(B.CSRC, SRC), flags)
    if os.path.exists(lib) and os.path.exists(stamp_file) and open(stamp_file).read() == stamp:
        return lib
    B.build()                                                   # the other objects (a no-op where they are up to date)
    os.makedirs(out_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = os.path.join(out_dir, "impl_slab.o")
    subprocess.check_call([hipcc] + flags + ["-c", os.path.join(B.CSRC, SRC), "-o", obj], stderr=subprocess.DEVNULL)
    objs = [obj if n == SRC else os.path.join(B.OBJDIR, n[:-4] + ".o") for n in B.sources()]
    subprocess.check_call([hipcc, "--offload-arch=" + B.ARCH, "-shared", "-fPIC", "-o", lib] + objs)
    with open(stamp_file, "w") as fh:
        fh.write(stamp)
    return lib


def _net(sd):
    from zeroshape_amd.model.shape.implicit import Implicit
    m = Implicit(syn.NUM_PATCHES, latent_dim=syn.LATENT_DIM, semantic=False, n_channels=syn.N_CHANNELS,
                 n_blocks_attn=syn.ATT_BLOCKS, n_layers_mlp=syn.MLP_LAYERS, num_heads=syn.NUM_HEADS,
                 posenc_3D=0, mlp_ratio=syn.MLP_RATIO, skip_in=list(syn.SKIP_IN), pos_perlayer=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _arm(monkeypatch, env):
    monkeypatch.delenv("ZS_SPLIT_BLOCK0_GEMM", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def cloud(m):
    """tests/test_gpu_split_ln_regs.py's lists; the 300-point one also holds a corner of the cube (|x| = |y| = |z| = 1.5) and
    the origin, in both images."""
    pts = torch.from_numpy(syn.seeded_cloud(200 + m, 2, m, -1.5, 1.5))
    if m == 300:
        pts[:, 7] = torch.tensor([1.5, -1.5, 1.5])
        pts[:, 131] = 0.0
    return pts.cuda()


@pytest.fixture(scope="module")
def ctx(seeded_sd):
    """The seeded network, two images with different latents, their split (calibrated) and exact states - prepared once with
    the tree's library, never modified - and the slab-form library, typed like the tree's."""
    from zeroshape_amd.model.shape.implicit import DecoderState
    regs = _lib.load()
    slab = ctypes.CDLL(build_slab_lib())
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(slab, name)
        fn.restype, fn.argtypes = res, args
    assert slab.zs_abi_version() == _lib.ABI_VERSION
    net = _net(seeded_sd)
    latent = torch.from_numpy(syn.seeded_latent(seed=0, batch=2)).cuda()
    assert not torch.equal(latent[0], latent[1])
    split, exact = net.prepare(latent), net.prepare(latent, "f32")
    return dict(net=net, latent=latent, split=split, exact=exact, libs={"regs": regs, "slab": slab},
                axis=torch.linspace(-1.5, 1.5, 33, device="cuda"),
                split1=DecoderState(split.programs[:1], 1, "f16x3", exact=exact.programs[:1]))


def _with(monkeypatch, ctx, build, launch):
    """launch() with the binding's handle on one of the two libraries (tools/ab_impl_regs.py does the same)."""
    monkeypatch.setattr(_lib, "_lib", ctx["libs"][build])
    out = launch().clone()
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "_lib", ctx["libs"]["regs"])
    return out


def test_calibration_still_selects_f16x3(ctx):
    assert ctx["split"].precision == "f16x3"


@pytest.mark.parametrize("arm", ARMS, ids=[a[0] for a in ARMS])
@pytest.mark.parametrize("images", [1, 2])
@pytest.mark.parametrize("m", [1, 33, 128, 129, 300])
def test_point_lists_bit_equal_to_the_slab_form_and_near_fp32(ctx, monkeypatch, m, images, arm):
    """Ragged last tiles (1, 33, 129, 300), a whole tile (128), one and two images."""
    from zeroshape_amd.model.shape.implicit import DecoderState
    net = ctx["net"]
    pts = cloud(m)[:images].contiguous()
    if m == 300:
        assert bool((pts.abs() == 1.5).all(dim=2).any()) and bool((pts == 0).all(dim=2).any())
    split = DecoderState(ctx["split"].programs[:images], images, "f16x3", exact=ctx["exact"].programs[:images])
    exact = net.query_points(DecoderState(ctx["exact"].programs[:images], images, "f32"), pts)
    _arm(monkeypatch, arm[1])
    got = _with(monkeypatch, ctx, "regs", lambda: net.query_points(split, pts))
    assert got.shape == (images, m) and int(net.last_tile_flags.sum()) == 0
    ref = _with(monkeypatch, ctx, "slab", lambda: net.query_points(split, pts))
    assert int(net.last_tile_flags.sum()) == 0
    err = float((got - exact).abs().max())
    print("m = %d, %d image(s), %s: %d of %d logits differ from the slab form; max |split - fp32| = %.3g at max |logit| = %.3g" %
          (m, images, arm[0], int((got != ref).sum()), got.numel(), err, float(exact.abs().max())))
    assert torch.equal(got, ref)
    assert err <= FP32_ATOL
    if images == 2:
        assert not torch.equal(got[0], got[1])                                # per-image latents are honoured


@pytest.mark.parametrize("arm", ARMS, ids=[a[0] for a in ARMS])
def test_grid33_bit_equal_to_the_slab_form_and_bit_reproducible(ctx, monkeypatch, arm):
    """35,937 points = 281 tiles on at most 256 workgroups: a tile count the grid does not divide.  Raw logits and
    occupancies equal the slab form's bit for bit, and two identical launches of the tree's library are bit-equal."""
    net, latent, axis, st = ctx["net"], ctx["latent"][:1], ctx["axis"], ctx["split1"]
    _arm(monkeypatch, arm[1])
    for sig in (False, True):
        got = _with(monkeypatch, ctx, "regs", lambda: net.query_grid(latent, axis, apply_sigmoid=sig, state=st))
        assert got.shape == (1, 33, 33, 33) and int(net.last_tile_flags.sum()) == 0
        ref = _with(monkeypatch, ctx, "slab", lambda: net.query_grid(latent, axis, apply_sigmoid=sig, state=st))
        again = _with(monkeypatch, ctx, "regs", lambda: net.query_grid(latent, axis, apply_sigmoid=sig, state=st))
        print("grid 33, %s, sigmoid %s: %d values differ from the slab form, %d between two launches" %
              (arm[0], sig, int((got != ref).sum()), int((got != again).sum())))
        assert torch.equal(got, ref)
        assert torch.equal(got, again)
