"""torch.autograd bindings of the HIP training kernels (include/zeroshape_hip.h, "Training").

Every op here is a torch.autograd.Function whose forward AND backward are launches of
libzeroshape_hip.so; torch supplies the tape, the tensor memory and the stream, nothing else.
Activations are fp32 channels-last ([B,H,W,C]; token matrices [B,L,C]), parameters stay in the
reference's torch layout ([Cout,Cin,kh,kw] / [Cout,Cin]) and are re-packed on the GPU when they
change (zs_pack_conv_weight; nn/operands.py owns the packed forms), so optimiser steps need no host work.

Reference behaviour reproduced: what torch.autograd gives train.py for Graph.forward(training=True)
(model/compute_graph/graph_shape.py:115-204) and Loss.shape_loss (utils/loss.py:18-28).
"""
import os

import torch

from .. import _lib
from . import ops
# The header's ZS_ACT_* / ZS_CONV_* values have one owner, nn/ops.py; ACT_* are here for this module's callers (A.ACT_RELU ...).
from .ops import ACT_GELU, ACT_NONE, ACT_RELU, ACT_RELU_CLAMP1, ACT_SOFTPLUS  # noqa: F401
from .ops import CONV_F16X3, CONV_IN_DILATE2, CONV_IN_RELU
from .pack import out_size
# The packed / standardised / split forms of the weights and the switches that choose among them have one owner, nn/operands.py;
# the second line of names is here for the callers outside nn/ (engines, optimiser, checkpoint loading, tools).
from .operands import CACHE, SWITCHES, ceil4
from .operands import GENERATION, bump_generation, refresh_packs, set_backward_precision, set_forward_precision  # noqa: F401

# Arithmetic of the weight-gradient GEMMs (zs_conv2d_wgrad with ZS_CONV_F16X3: wgrad_split_kernel, round 3).  Follows the
# data-gradient setting (optim.amp) unless ZS_TRAIN_WGRAD_PRECISION pins it (A/B measurements).  It stays beside its one reader,
# _Conv.backward: a weight gradient reads activations and gradients, no cached operand, so no operand's stamp depends on it.
BWD_WGRAD_PRECISION = os.environ.get("ZS_TRAIN_WGRAD_PRECISION")


def wgrad_precision():
    return BWD_WGRAD_PRECISION or SWITCHES.backward


def _stream(t):
    return _lib.current_stream_ptr(t.device)


def _f32c(t, what):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise ValueError("%s: fp32 GPU tensor required (zeroshape_amd has no CPU path)" % what)
    return t if t.is_contiguous() else t.contiguous()


# ---- scratch buffers (grow-only, one per device and purpose; launches on one stream serialise) ----
_SCRATCH = {}


SCRATCH_GENERATION = [0]     # bumped when a workspace is (re)allocated: a captured step holds the old address


_WS_BYTES = {}      # (query, args) -> bytes: the *_workspace_bytes queries are pure functions of their arguments


def _ws_bytes(query, *args):
    """A workspace-size query of the C ABI, asked once per argument tuple (a training step made 459 such calls - a quarter of
    its C-ABI calls - for sizes that never change)."""
    key = (query,) + args
    n = _WS_BYTES.get(key)
    if n is None:
        n = _WS_BYTES[key] = int(getattr(_lib.load(), query)(*args))
    return n


def scratch(device, name, nbytes):
    key = (str(device), name)
    n = (int(nbytes) + 3) // 4
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 1), dtype=torch.float32, device=device)
        _SCRATCH[key] = buf
        SCRATCH_GENERATION[0] += 1
    return buf


def _conv_launch(x, rec, shift, res1, res2, out, kh, kw, stride, pt, pl, flags, in_scale, in_shift, act):
    lib = _lib.load()
    B, H, W, C = x.shape
    _, Ho, Wo, Co = out.shape
    packed, flags = CACHE.operand(rec, flags, B * Ho * Wo, C, Co, kh, kw, in_scale, in_shift)
    with _lib.on(x.device):
        _lib.check(lib.zs_conv2d_nhwc(_lib.ptr(x), _lib.ptr(packed), None, _lib.ptr(shift), _lib.ptr(res1),
                                      _lib.ptr(res2), _lib.ptr(out), B, H, W, C, Ho, Wo, Co, kh, kw, stride, pt, pl,
                                      flags, float(in_scale), float(in_shift), act, _stream(x)), "zs_conv2d_nhwc")


def column_sum(x2d, scale=1.0):
    """[rows, C] -> [C]."""
    lib = _lib.load()
    rows, C = x2d.shape
    out = torch.empty(C, dtype=torch.float32, device=x2d.device)
    ws = scratch(x2d.device, "colsum", _ws_bytes("zs_column_sum_workspace_bytes", rows, C))
    with _lib.on(x2d.device):
        _lib.check(lib.zs_column_sum(_lib.ptr(x2d), _lib.ptr(out), rows, C, float(scale), _lib.ptr(ws), _stream(x2d)),
                   "zs_column_sum")
    return out


def _act_backward(dy, ref, act, beta=0.0):
    lib = _lib.load()
    dx = torch.empty_like(dy)
    with _lib.on(dy.device):
        _lib.check(lib.zs_act_backward(_lib.ptr(dy), _lib.ptr(ref), _lib.ptr(dx), dy.numel(), act, float(beta),
                                       _stream(dy)), "zs_act_backward")
    return dx


# Segmented backward (the captured training step on more than one GPU, model/shape_engine.py).  One hipGraph of forward +
# backward leaves the bucket all-reduce nothing to overlap with: every gradient appears "at once" when the replay ends.  So
# the forward marks a few places where the network can be CUT (A.cut / A.segment_break, no-ops unless a segmenting capture
# is active): a cut tensor is handed to the consumers of LATER segments as a detached leaf, so torch.autograd can run the
# backward pass one segment at a time - backward_segment(s) starts from the cut tensors segment s produced, with the
# gradients their leaves collected, and stops at the leaves of earlier segments - each segment captured into its own
# hipGraph.  Between two replays the engine packs and all-reduces the buckets whose gradients are final while the next
# segment's backward runs (parallel.GradReducer.launch_done).  The arithmetic is the unsegmented step's: a cut adds no
# operation, and a tensor with consumers on both sides of a cut receives the same two-term gradient sum.
SEGMENTS = None               # {"index": current segment, "cuts": [(producer segment, tensor, detached leaf)]} while segmenting


def begin_segments():
    global SEGMENTS
    SEGMENTS = {"index": 0, "cuts": []}


def end_segments():
    global SEGMENTS
    SEGMENTS = None


def segment_break():
    """The forward moves on to the next segment (everything computed from here on may only read earlier segments' tensors
    through cut())."""
    if SEGMENTS is not None:
        SEGMENTS["index"] += 1


def cut(*tensors):
    """The tensors as LATER segments must read them: detached leaves that collect their gradient (the same storage - no copy);
    the originals stay usable inside the segment that produced them.  Identity when no segmenting capture is active, and for
    tensors that carry no gradient."""
    out = []
    for x in tensors:
        if SEGMENTS is not None and torch.is_tensor(x) and x.requires_grad:
            leaf = x.detach().requires_grad_()
            SEGMENTS["cuts"].append((SEGMENTS["index"], x, leaf))
            x = leaf
        out.append(x)
    return out[0] if len(out) == 1 else tuple(out)


def segment_has_work(s):
    """Does segment s have anything to differentiate (a cut tensor it produced that collected a gradient)?"""
    return any(seg == s and leaf.grad is not None for seg, _, leaf in SEGMENTS["cuts"])


def backward_segment(s, params, loss=None):
    """Backward pass of segment s: from `loss` (the last segment) and from the cut tensors segment s produced - seeded with
    what their leaves collected in the later segments - to the parameters (those of other segments are unreachable and
    skipped) and the leaves cut by earlier segments.  -> False when the segment has nothing to differentiate."""
    roots, grads = ([loss], [None]) if loss is not None else ([], [])
    for seg, x, leaf in SEGMENTS["cuts"]:
        if seg == s and leaf.grad is not None:
            roots.append(x)
            grads.append(leaf.grad)
    inputs = list(params) + [leaf for seg, _, leaf in SEGMENTS["cuts"] if seg < s]
    if not roots or not inputs:
        return False
    torch.autograd.backward(roots, grads, inputs=inputs)
    return True


def _posenc3d_forward(pts, L):
    lib = _lib.load()
    cpad = (3 + 6 * L + 3) // 4 * 4
    out = torch.empty(*pts.shape[:-1], cpad, dtype=torch.float32, device=pts.device)
    with _lib.on(pts.device):
        _lib.check(lib.zs_posenc3d(_lib.ptr(pts), pts.numel() // 3, int(L), _lib.ptr(out), cpad, _stream(pts)), "zs_posenc3d")
    return out


def _first_order_only(what):
    """Inside a backward: the kernels behind this module's Functions record no graph of their own, so a backward pass that is
    itself being recorded (create_graph=True) would hand out gradients that look differentiable and are constants."""
    if torch.is_grad_enabled():
        raise RuntimeError("%s: first-order gradient only - torch.autograd was asked for a differentiable backward pass "
                           "(create_graph=True), which the HIP kernels do not provide" % what)


class _PosEnc3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, L):
        pts = _f32c(points, "posenc3d input")
        ctx.L = L
        ctx.save_for_backward(pts)
        return _posenc3d_forward(pts, L)

    @staticmethod
    def backward(ctx, denc):
        _first_order_only("posenc3d")
        (pts,) = ctx.saved_tensors
        return ops.posenc3d_bwd(pts, ctx.L, _f32c(denc, "posenc3d grad")), None


def posenc3d(points, L):
    """points [..., 3] -> NeRF encoding [..., pad4(3 + 6 L)], the reference's get_embedder(L, 3) (utils/layers.py:8-53), channels
    beyond 3 + 6 L zero (the channel count the GEMM stages).  Points that carry a gradient get it back through zs_posenc3d_bwd;
    points that do not (training: the query points are data) cost the one launch and save nothing."""
    if torch.is_grad_enabled() and points.requires_grad:
        return _PosEnc3D.apply(points, L)
    return _posenc3d_forward(_f32c(points.detach(), "posenc3d input"), L)


class _QueryPoints(torch.autograd.Function):
    """The identity on query points that carry a gradient, at the head of Implicit's layer-by-layer path: its backward is where
    a create_graph=True request for the point gradient fails loudly (whatever the configuration puts behind it)."""

    @staticmethod
    def forward(ctx, points):
        return points.view_as(points)

    @staticmethod
    def backward(ctx, dpoints):
        _first_order_only("Implicit: the gradient w.r.t. points_3D")
        return dpoints


def query_points(points):
    return _QueryPoints.apply(points) if torch.is_grad_enabled() and points.requires_grad else points


class side_state(object):
    """Within the block this module's launches use scratch buffers and an operand cache of their own (kept between blocks),
    and SCRATCH_GENERATION reads afterwards what it read before: a captured training step - which holds the addresses of the
    main scratch buffers and the launch tables of the main cache - is not invalidated by work that is not a training step
    (Implicit.field_gradient: other row counts, data gradients training never asks for)."""
    _scratch, _cache = {}, None

    def __enter__(self):
        global _SCRATCH, CACHE
        if side_state._cache is None:
            side_state._cache = type(CACHE)()
        self.saved = (_SCRATCH, CACHE, SCRATCH_GENERATION[0])
        _SCRATCH, CACHE = side_state._scratch, side_state._cache
        return self

    def __exit__(self, *exc):
        global _SCRATCH, CACHE
        _SCRATCH, CACHE, SCRATCH_GENERATION[0] = self.saved
        return False


class _PadChannels(torch.autograd.Function):
    """[..., C] -> [..., cpad] with zero padding channels (the channel count the convolution engine stages)."""

    @staticmethod
    def forward(ctx, x, cpad):
        ctx.C = x.shape[-1]
        return ops.pad_channels(_f32c(x, "pad input"), cpad)

    @staticmethod
    def backward(ctx, dy):
        return dy[..., :ctx.C].contiguous(), None


def pad_channels(x, cpad):
    return x if x.shape[-1] == cpad else _PadChannels.apply(x, cpad)


class _Conv(torch.autograd.Function):
    """y = act(conv(T(x), W[:, cin0:cin0+cin]) + bias + res1 + res2), T = input ReLU / affine."""

    @staticmethod
    def forward(ctx, x, weight, bias, res1, res2, cfg):
        x = _f32c(x, "conv input")
        stride, padding, act = cfg["stride"], cfg["padding"], cfg["act"]
        assert act in (ACT_NONE, ACT_RELU, ACT_RELU_CLAMP1), "fuse only ReLU-type activations when training"
        B, H, W, Cx = x.shape
        cout = weight.shape[0]
        kh, kw = (weight.shape[2], weight.shape[3]) if weight.dim() == 4 else (1, 1)
        cin0 = cfg.get("cin0", 0)
        cin = cfg.get("cin") or weight.shape[1]
        assert Cx == ceil4(cin), "input has %d channels, layer expects %d (padded to 4)" % (Cx, cin)
        std_eps = cfg.get("std_eps")
        Ho, pt = out_size(H, kh, stride, padding)
        Wo, pl = out_size(W, kw, stride, padding)
        out = torch.empty(B, Ho, Wo, cout, dtype=torch.float32, device=x.device)
        flags = (CONV_IN_RELU if cfg.get("in_relu") else 0) | (CONV_F16X3 if SWITCHES.forward == "f16x3" else 0)
        _conv_launch(x, CACHE.pack(weight, cin0, cin, False, std_eps), None if bias is None else bias.detach(),
                     None if res1 is None else _f32c(res1, "res1"), None if res2 is None else _f32c(res2, "res2"),
                     out, kh, kw, stride, pt, pl, flags, cfg.get("in_scale", 1.0), cfg.get("in_shift", 0.0), act)
        ctx.cfg = dict(cfg, pt=pt, pl=pl, kh=kh, kw=kw, cin0=cin0, cin=cin)
        ctx.has = (bias is not None, res1 is not None, res2 is not None)
        ctx.save_for_backward(x, weight, out if act != ACT_NONE else None)
        return (out, x.view_as(x)) if cfg.get("fork") else out

    @staticmethod
    def backward(ctx, dy, dpass=None):
        lib = _lib.load()
        x, weight, out = ctx.saved_tensors
        if dpass is not None:
            dpass = _f32c(dpass, "conv pass-through grad")
        cfg = ctx.cfg
        kh, kw, stride, pt, pl = cfg["kh"], cfg["kw"], cfg["stride"], cfg["pt"], cfg["pl"]
        cin0, cin, act = cfg["cin0"], cfg["cin"], cfg["act"]
        in_relu, in_scale, in_shift = bool(cfg.get("in_relu")), cfg.get("in_scale", 1.0), cfg.get("in_shift", 0.0)
        std_eps = cfg.get("std_eps")
        g = _f32c(dy, "conv grad")
        if act != ACT_NONE:
            g = _act_backward(g, out, act)
        B, Ho, Wo, cout = g.shape
        _, H, W, Cx = x.shape
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        want_b = ctx.has[0] and need_b
        gp = g if cout % 4 == 0 else ops.pad_channels(g, ceil4(cout))
        dw = db = None
        if want_b and not need_w:
            db = column_sum(g.view(-1, cout))
        if need_w:
            sub = cin != weight.shape[1]
            dw = torch.zeros_like(weight) if sub else torch.empty_like(weight)
            if want_b:          # the bias gradient rides on the weight-gradient kernel (it stages dY anyway)
                db = torch.empty(cout, dtype=torch.float32, device=x.device)
            flags = (CONV_IN_RELU if in_relu else 0) | (CONV_F16X3 if wgrad_precision() == "f16x3" else 0)
            ws = scratch(x.device, "wgrad", _ws_bytes("zs_conv2d_wgrad_workspace_bytes", B, Ho, Wo, Cx, cout, kh, kw))
            with _lib.on(x.device):
                _lib.check(lib.zs_conv2d_wgrad(_lib.ptr(x), _lib.ptr(gp), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), B, H, W, Cx, Ho,
                                               Wo, cout, kh, kw, stride, pt, pl, flags, float(in_scale),
                                               float(in_shift), cin, cin0, weight.shape[1], 0, _stream(x)),
                           "zs_conv2d_wgrad")
            if std_eps is not None:
                dws = torch.empty_like(weight)
                with _lib.on(x.device):
                    _lib.check(lib.zs_standardize_weight_bwd(_lib.ptr(weight.detach()), _lib.ptr(dw), _lib.ptr(dws),
                                                             weight.shape[0], weight[0].numel(), float(std_eps),
                                                             _stream(x)), "zs_standardize_weight_bwd")
                dw = dws
        dx = None
        if need_x:
            assert stride in (1, 2), "data gradient: stride 1 or 2"
            if cin <= 4 and cout % 4 == 0 and kh * kw * cout * 16 <= 160 * 1024:
                # a network stem: direct gather kernel instead of a GEMM with 3 useful columns
                w_used = CACHE.standardize(weight, std_eps) if std_eps is not None else weight.detach()
                dx = torch.empty(B, H, W, Cx, dtype=torch.float32, device=x.device)
                with _lib.on(x.device):
                    _lib.check(lib.zs_conv2d_dgrad_small_cin(_lib.ptr(g), _lib.ptr(w_used), _lib.ptr(dx), B, H, W, Cx, Ho, Wo,
                                                             cout, kh, kw, stride, pt, pl, cin, cin0, weight.shape[1],
                                                             float(in_scale), _stream(x)), "zs_conv2d_dgrad_small_cin")
            else:
                dx = torch.empty(B, H, W, cin, dtype=torch.float32, device=x.device)
                flags = (CONV_IN_DILATE2 if stride == 2 else 0) | (CONV_F16X3 if SWITCHES.backward == "f16x3" else 0)
                fused = dpass is not None and cin == Cx and not in_relu     # the pass-through's gradient: the GEMM's residual
                _conv_launch(gp, CACHE.pack(weight, cin0, cin, True, std_eps), None, dpass if fused else None, None, dx, kh, kw, 1,
                             kh - 1 - pt, kw - 1 - pl, flags, in_scale, 0.0, ACT_NONE)
                if fused:
                    dpass = None
                if cin != Cx:                       # the input carried zero padding channels
                    dx = ops.pad_channels(dx, Cx)
            if in_relu:
                dx = _act_backward(dx, x, ACT_RELU)
        if dpass is not None:
            dx = dpass if dx is None else dx + dpass
        return dx, dw, db, (g if ctx.has[1] else None), (g if ctx.has[2] else None), None


def conv2d(x, weight, bias=None, stride=1, padding=0, act=ACT_NONE, in_relu=False, in_scale=1.0, in_shift=0.0,
           res1=None, res2=None, std_eps=None, cin0=0, cin=None, fork=False):
    """fork=True: returns (conv(x), x) - see "Forks" below; x's other consumer takes the returned x."""
    cfg = dict(stride=stride, padding=padding, act=act, in_relu=in_relu, in_scale=in_scale, in_shift=in_shift,
               std_eps=std_eps, cin0=cin0, cin=cin, fork=bool(fork) and FUSE_FORKS)
    y = _Conv.apply(x, weight, bias, res1, res2, cfg)
    return (y, x) if fork and not FUSE_FORKS else y


def linear(x, weight, bias=None, act=ACT_NONE, res1=None, in_scale=1.0, cin0=0, cin=None):
    """x [..., CinP] -> [..., Cout]."""
    lead = x.shape[:-1]
    n = 1
    for d in lead:
        n *= d
    y = conv2d(x.reshape(1, 1, n, x.shape[-1]), weight, bias, act=act, in_scale=in_scale, cin0=cin0, cin=cin,
               res1=None if res1 is None else res1.reshape(1, 1, n, weight.shape[0]))
    return y.view(*lead, weight.shape[0])


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, beta):
        lib = _lib.load()
        x = _f32c(x, "activation input")
        y = torch.empty_like(x)
        with _lib.on(x.device):
            _lib.check(lib.zs_act_forward(_lib.ptr(x), _lib.ptr(y), x.numel(), act, float(beta), _stream(x)),
                       "zs_act_forward")
        ctx.act, ctx.beta = act, beta
        ctx.save_for_backward(y if act in (ACT_RELU, ACT_RELU_CLAMP1) else x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (ref,) = ctx.saved_tensors
        return _act_backward(_f32c(dy, "activation grad"), ref, ctx.act, ctx.beta), None, None


def gelu(x):
    return _Act.apply(x, ACT_GELU, 0.0)


def softplus(x, beta=100.0):
    return _Act.apply(x, ACT_SOFTPLUS, beta)


def relu(x):
    return _Act.apply(x, ACT_RELU, 0.0)


# Forks.  A tensor with two consumers (x -> [norm / conv -> branch] and x -> residual add) receives two gradients, which
# the autograd engine sums with an elementwise launch of its own (~95 per training step of the shape graph, 4 us each).
# With fork=True the first consumer also hands x through (`y, x = op(x, fork=True)`, the second consumer takes THAT x):
# the pass-through's gradient arrives in the op's backward, which adds it inside the kernel that writes dx anyway
# (zs_layer_norm_bwd_add; the data-gradient GEMM's residual operand), and x's producer sees ONE gradient.
FUSE_FORKS = os.environ.get("ZS_TRAIN_FUSE_FORKS", "1") != "0"      # A/B switch: off = the pass-through is x itself


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, fork):
        x = _f32c(x, "layer_norm input")
        y = ops.layer_norm(x, gamma.detach(), beta.detach(), eps)
        ctx.eps = eps
        ctx.save_for_backward(x, gamma)
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, dy, dpass=None):
        lib = _lib.load()
        x, gamma = ctx.saved_tensors
        dy = _f32c(dy, "layer_norm grad")
        add = None if dpass is None else _f32c(dpass, "layer_norm pass-through grad")
        C = x.shape[-1]
        rows = x.numel() // C
        dx = torch.empty_like(x)
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = scratch(x.device, "ln_bwd", _ws_bytes("zs_layer_norm_bwd_workspace_bytes", rows, C))
        with _lib.on(x.device):
            _lib.check(lib.zs_layer_norm_bwd_add(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(gamma.detach()), _lib.ptr(add),
                                                 _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db), rows, C, float(ctx.eps),
                                                 _lib.ptr(ws), _stream(x)), "zs_layer_norm_bwd_add")
        return dx, dg, db, None, None


def layer_norm(x, gamma, beta, eps=1e-6, fork=False):
    """fork=True: returns (LayerNorm(x), x) - see "Forks" above."""
    if not fork:
        return _LayerNorm.apply(x, gamma, beta, eps, False)
    if not FUSE_FORKS:
        return _LayerNorm.apply(x, gamma, beta, eps, False), x
    return _LayerNorm.apply(x, gamma, beta, eps, True)


ATT_FWD_SPLIT = os.environ.get("ZS_TRAIN_ATT_SPLIT", "1") != "0"      # A/B switch


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads):
        qkv = _f32c(qkv, "attention input")
        # optim.amp: the split-fp16 forms, like the forward GEMMs around it (batch 4 = 48 (sample, head) pairs: the key-split
        # kernel, 25 -> 9 us per ViT block); the backward pass recomputes the probabilities in fp32 either way.  The choice is
        # this path's own (passed explicitly): it never follows the inference switch ops.CONV_PRECISION
        out = ops.attention(qkv, heads, split=SWITCHES.forward == "f16x3" and ATT_FWD_SPLIT)
        ctx.heads = heads
        ctx.save_for_backward(qkv)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        (qkv,) = ctx.saved_tensors
        dout = _f32c(dout, "attention grad")
        B, L, C3 = qkv.shape
        heads = ctx.heads
        dqkv = torch.empty_like(qkv)
        ws = scratch(qkv.device, "attn_bwd", _ws_bytes("zs_attention_bwd_workspace_bytes", B, L, heads))
        with _lib.on(qkv.device):
            _lib.check(lib.zs_attention_bwd(_lib.ptr(qkv), _lib.ptr(dout), _lib.ptr(dqkv), _lib.ptr(ws), B, L, heads,
                                            C3 // 3 // heads, _stream(qkv)), "zs_attention_bwd")
        return dqkv, None


def attention(qkv, heads):
    return _Attention.apply(qkv, heads)


class _PointAttention(torch.autograd.Function):
    """ImplFuncAttention's point rows (implicit.py:44-66): softmax over the latent keys + self."""

    @staticmethod
    def forward(ctx, qkv_p, qkv_l, heads):
        lib = _lib.load()
        qkv_p, qkv_l = _f32c(qkv_p, "point qkv"), _f32c(qkv_l, "latent qkv")
        B, M, C3 = qkv_p.shape
        Ll, C = qkv_l.shape[1], C3 // 3
        out = torch.empty(B, M, C, dtype=torch.float32, device=qkv_p.device)
        with _lib.on(qkv_p.device):
            _lib.check(lib.zs_point_attention(_lib.ptr(qkv_p), _lib.ptr(qkv_l), _lib.ptr(out), B, M, Ll, heads,
                                              C // heads, _stream(qkv_p)), "zs_point_attention")
        ctx.heads = heads
        ctx.save_for_backward(qkv_p, qkv_l)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        qkv_p, qkv_l = ctx.saved_tensors
        dout = _f32c(dout, "point attention grad")
        B, M, C3 = qkv_p.shape
        Ll, C, heads = qkv_l.shape[1], C3 // 3, ctx.heads
        dp, dl = torch.empty_like(qkv_p), torch.empty_like(qkv_l)
        ws = scratch(qkv_p.device, "pa_bwd", _ws_bytes("zs_point_attention_bwd_workspace_bytes", B, M, Ll, heads))
        with _lib.on(qkv_p.device):
            _lib.check(lib.zs_point_attention_bwd(_lib.ptr(qkv_p), _lib.ptr(qkv_l), _lib.ptr(dout), _lib.ptr(dp),
                                                  _lib.ptr(dl), 0, _lib.ptr(ws), B, M, Ll, heads, C // heads,
                                                  _stream(qkv_p)), "zs_point_attention_bwd")
        return dp, dl, None


def point_attention(qkv_p, qkv_l, heads):
    return _PointAttention.apply(qkv_p, qkv_l, heads)


def point_attention_probs(qkv_p, qkv_l, heads, attn, weight=1.0, accumulate=False):
    """attn [B,M,Ll] (=|+=) weight * mean over the heads of the points' softmax probabilities over the latent tokens (the
    attention map the reference returns, implicit.py:60-66,277).  No gradient (visualisation only)."""
    lib = _lib.load()
    qp, ql = _f32c(qkv_p.detach(), "qkv points"), _f32c(qkv_l.detach(), "qkv latent")
    B, M, Ll = qp.shape[0], qp.shape[1], ql.shape[1]
    assert attn.shape == (B, M, Ll) and attn.is_contiguous() and attn.dtype == torch.float32
    with _lib.on(qp.device):
        _lib.check(lib.zs_point_attention_probs(_lib.ptr(qp), _lib.ptr(ql), _lib.ptr(attn), B, M, Ll, heads, qp.shape[-1] // (3 * heads),
                                                float(weight), 1 if accumulate else 0, _stream(qp)), "zs_point_attention_probs")
    return attn


def _scaled_rows(x, branch, scale):
    lib = _lib.load()
    B = branch.shape[0]
    y = torch.empty_like(branch)
    with _lib.on(branch.device):
        _lib.check(lib.zs_add_scaled_rows(_lib.ptr(x), _lib.ptr(branch), _lib.ptr(scale), _lib.ptr(y), B,
                                          branch.numel() // B, _stream(branch)), "zs_add_scaled_rows")
    return y


class _AddScaledRows(torch.autograd.Function):
    """x + scale[b] * branch: residual connection under per-sample stochastic depth (timm DropPath)."""

    @staticmethod
    def forward(ctx, x, branch, scale):
        x, branch = _f32c(x, "residual"), _f32c(branch, "branch")
        ctx.save_for_backward(scale)
        return _scaled_rows(x, branch, scale)

    @staticmethod
    def backward(ctx, dy):
        (scale,) = ctx.saved_tensors
        dy = _f32c(dy, "residual grad")
        return dy, _scaled_rows(None, dy, scale), None


def add_scaled_rows(x, branch, scale):
    return _AddScaledRows.apply(x, branch, _f32c(scale, "drop-path scale"))


class _BCELogits(torch.autograd.Function):
    """Loss.shape_loss (utils/loss.py:18-28): mean of w * BCEWithLogits(pred, sdf < 0)."""

    @staticmethod
    def forward(ctx, logits, sdf, thres, weight):
        lib = _lib.load()
        logits, sdf = _f32c(logits, "logits"), _f32c(sdf, "sdf")
        n = logits.numel()
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        ws = scratch(logits.device, "bce", _ws_bytes("zs_bce_logits_workspace_bytes", n))
        with _lib.on(logits.device):
            _lib.check(lib.zs_bce_logits(_lib.ptr(logits), _lib.ptr(sdf), n, float(thres), float(weight),
                                         _lib.ptr(loss), _lib.ptr(ws), _stream(logits)), "zs_bce_logits")
        ctx.thres, ctx.weight = thres, weight
        ctx.save_for_backward(logits, sdf)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        logits, sdf = ctx.saved_tensors
        dloss = _f32c(dloss, "loss grad")
        dx = torch.empty_like(logits)
        with _lib.on(logits.device):
            _lib.check(lib.zs_bce_logits_bwd(_lib.ptr(logits), _lib.ptr(sdf), logits.numel(), float(ctx.thres),
                                             float(ctx.weight), _lib.ptr(dloss), _lib.ptr(dx), _stream(logits)),
                       "zs_bce_logits_bwd")
        return dx, None, None, None


def bce_logits(logits, sdf, impt_thres=0.01, impt_weight=1.0):
    return _BCELogits.apply(logits, sdf, impt_thres, impt_weight)


# =============================================================================================
# Encoder layers: BatchNorm (training), GroupNorm, pooling, resampling, layout, geometry
# =============================================================================================
class _BatchNormTrain(torch.autograd.Function):
    """nn.BatchNorm2d in training mode over channels-last x (+ residual, ReLU fused): batch
    statistics, running-stat update (momentum, unbiased variance) as torch does."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, eps, momentum, relu):
        lib = _lib.load()
        x = _f32c(x, "batch_norm input")
        C = x.shape[-1]
        rows = x.numel() // C
        y = torch.empty_like(x)
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        rstd = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = scratch(x.device, "bn", _ws_bytes("zs_batch_norm_workspace_bytes", rows, C))
        res = None if residual is None else _f32c(residual, "batch_norm residual")
        with _lib.on(x.device):
            _lib.check(lib.zs_batch_norm_train(_lib.ptr(x), _lib.ptr(gamma.detach()), _lib.ptr(beta.detach()),
                                               _lib.ptr(res), _lib.ptr(y), _lib.ptr(running_mean),
                                               _lib.ptr(running_var), _lib.ptr(mean), _lib.ptr(rstd), rows, C,
                                               float(eps), float(momentum), 1 if relu else 0, _lib.ptr(ws),
                                               _stream(x)), "zs_batch_norm_train")
        ctx.relu, ctx.has_res = relu, residual is not None
        ctx.save_for_backward(x, gamma, mean, rstd, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gamma, mean, rstd, y = ctx.saved_tensors
        dy = _f32c(dy, "batch_norm grad")
        C = x.shape[-1]
        rows = x.numel() // C
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if (ctx.has_res and ctx.relu) else None
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = scratch(x.device, "bn", _ws_bytes("zs_batch_norm_workspace_bytes", rows, C))
        with _lib.on(x.device):
            _lib.check(lib.zs_batch_norm_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(y), _lib.ptr(gamma.detach()),
                                             _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(dx), _lib.ptr(dres), _lib.ptr(dg),
                                             _lib.ptr(db), rows, C, _lib.ptr(ws), _stream(x)), "zs_batch_norm_bwd")
        if ctx.has_res and not ctx.relu:
            dres = dy
        return dx, dg, db, dres, None, None, None, None, None


_BN_COUNTERS = [None]      # inside deferred_bn_counters(): the num_batches_tracked buffers to bump on exit


class deferred_bn_counters(object):
    """Within the block batch_norm_train() only notes the layers' `num_batches_tracked` buffers; on exit they are all
    incremented by ONE multi-tensor launch (a training forward of the shape graph has 66 BatchNorm layers: 66 one-element
    kernels, 0.27 ms of a 27 ms step).  Re-entrant: an inner block leaves the flush to the outermost one."""

    def __enter__(self):
        self.outer = _BN_COUNTERS[0] is not None
        if not self.outer:
            _BN_COUNTERS[0] = []
        return self

    def __exit__(self, *exc):
        if not self.outer:
            pending, _BN_COUNTERS[0] = _BN_COUNTERS[0], None
            # flushed whether or not an exception leaves the block: the counters describe running-statistics updates that
            # already happened in place (a BatchNorm with momentum=None averages over exactly this count - ADVICE r05)
            if pending:
                torch._foreach_add_(pending, 1)
        return False


def batch_norm_train(x, bn, relu=False, residual=None):
    """bn: an nn.BatchNorm2d in training mode (its running statistics are updated in place)."""
    momentum = 0.1 if bn.momentum is None else bn.momentum
    y = _BatchNormTrain.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, bn.eps, momentum, relu)
    if bn.num_batches_tracked is not None:
        if _BN_COUNTERS[0] is not None:
            _BN_COUNTERS[0].append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked += 1
    return y


class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, groups, eps, relu):
        lib = _lib.load()
        x = _f32c(x, "group_norm input")
        B, H, W, C = x.shape
        y = torch.empty_like(x)
        res = None if residual is None else _f32c(residual, "group_norm residual")
        with _lib.on(x.device):
            _lib.check(lib.zs_group_norm_nhwc(_lib.ptr(x), _lib.ptr(gamma.detach()), _lib.ptr(beta.detach()),
                                              _lib.ptr(res), _lib.ptr(y), B, H * W, C, groups, float(eps),
                                              1 if relu else 0, _stream(x)), "zs_group_norm_nhwc")
        ctx.cfg = (groups, eps, relu, residual is not None)
        ctx.save_for_backward(x, gamma, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, gamma, y = ctx.saved_tensors
        groups, eps, relu, has_res = ctx.cfg
        dy = _f32c(dy, "group_norm grad")
        B, H, W, C = x.shape
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if (has_res and relu) else None
        dg = torch.empty(C, dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = scratch(x.device, "gn_bwd", _ws_bytes("zs_group_norm_bwd_workspace_bytes", B, C))
        with _lib.on(x.device):
            _lib.check(lib.zs_group_norm_bwd(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(y), _lib.ptr(gamma.detach()),
                                             _lib.ptr(dx), _lib.ptr(dres), _lib.ptr(dg), _lib.ptr(db), B, H * W, C,
                                             groups, float(eps), _lib.ptr(ws), _stream(x)), "zs_group_norm_bwd")
        if has_res and not relu:
            dres = dy
        return dx, dg, db, dres, None, None, None


def group_norm(x, gamma, beta, groups=32, eps=1e-5, relu=False, residual=None):
    return _GroupNorm.apply(x, gamma, beta, residual, groups, eps, relu)


class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, stride, padding):
        x = _f32c(x, "max_pool input")
        Ho, pt = out_size(x.shape[1], k, stride, padding)
        Wo, pl = out_size(x.shape[2], k, stride, padding)
        ctx.cfg = (k, stride, pt, pl, Ho, Wo)
        ctx.save_for_backward(x)
        return ops.max_pool(x, k, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        k, stride, pt, pl, Ho, Wo = ctx.cfg
        dy = _f32c(dy, "max_pool grad")
        B, H, W, C = x.shape
        dx = torch.empty_like(x)
        with _lib.on(x.device):
            _lib.check(lib.zs_max_pool_bwd_nhwc(_lib.ptr(x), _lib.ptr(dy), _lib.ptr(dx), B, H, W, C, Ho, Wo, k, stride,
                                                pt, pl, _stream(x)), "zs_max_pool_bwd_nhwc")
        return dx, None, None, None


def max_pool(x, k=3, stride=2, padding=1):
    return _MaxPool.apply(x, k, stride, padding)


class _GlobalMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x, "global_mean input")
        ctx.shape = tuple(x.shape)
        return ops.global_mean(x)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        B, H, W, C = ctx.shape
        dy = _f32c(dy, "global_mean grad")
        dx = torch.empty(B, H, W, C, dtype=torch.float32, device=dy.device)
        with _lib.on(dy.device):
            _lib.check(lib.zs_global_mean_bwd_nhwc(_lib.ptr(dy), _lib.ptr(dx), B, H * W, C, _stream(dy)),
                       "zs_global_mean_bwd_nhwc")
        return dx


def global_mean(x):
    return _GlobalMean.apply(x)


class _Upsample2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x, "upsample2x input")
        ctx.shape = tuple(x.shape)
        return ops.upsample2x(x)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        B, H, W, C = ctx.shape
        dy = _f32c(dy, "upsample2x grad")
        dx = torch.empty(B, H, W, C, dtype=torch.float32, device=dy.device)
        with _lib.on(dy.device):
            _lib.check(lib.zs_upsample2x_bwd_nhwc(_lib.ptr(dy), _lib.ptr(dx), B, H, W, C, _stream(dy)),
                       "zs_upsample2x_bwd_nhwc")
        return dx


def upsample2x(x):
    return _Upsample2x.apply(x)


class _ToNHWC(torch.autograd.Function):
    """NCHW [B,C,H,W] (times an optional per-pixel mask [B,1,H,W]) -> channels-last, zero padded to cpad."""

    @staticmethod
    def forward(ctx, x, mask, cpad):
        x = _f32c(x, "to_nhwc input")
        # the fp32 mask is converted here, once: the backward saves it, ops.to_nhwc finds nothing left to convert
        m = None if mask is None else _f32c(mask.float(), "to_nhwc mask")
        ctx.shape = tuple(x.shape) + (cpad,)
        ctx.save_for_backward(m)
        return ops.to_nhwc(x, cpad, m)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (m,) = ctx.saved_tensors
        B, C, H, W, cpad = ctx.shape
        dy = _f32c(dy, "to_nhwc grad")
        dx = torch.empty(B, C, H, W, dtype=torch.float32, device=dy.device)
        with _lib.on(dy.device):
            _lib.check(lib.zs_nhwc_to_nchw_masked(_lib.ptr(dy), _lib.ptr(m), _lib.ptr(dx), B, C, H * W, cpad,
                                                  _stream(dy)), "zs_nhwc_to_nchw_masked")
        return dx, None, None


def to_nhwc(x, cpad=None, mask=None):
    return _ToNHWC.apply(x, mask, cpad or x.shape[1])


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.to_nchw(_f32c(x, "to_nchw input"))

    @staticmethod
    def backward(ctx, dy):
        return ops.to_nhwc(_f32c(dy, "to_nchw grad"))


def to_nchw(x):
    return _ToNCHW.apply(x)


class _SeenSurface(torch.autograd.Function):
    """graph_shape.py:131-144 in one launch each way: (depth [B,1,H,W], intr [B,3,3], mask) ->
    (seen_points [B,HW,3], seen_3D_dsp [B,3,H/dsp,W/dsp], mask_dsp [B,1,H/dsp,W/dsp]).  dsp = 1: same-size resample;
    dsp = 2 (arch.depth.dsp = 2, the transformer coordinate encoder): the coordinate map and its mask resampled to half
    the size (interpolate_coordmap, utils/util.py:336-345)."""

    @staticmethod
    def forward(ctx, depth, intr, mask, dsp):
        lib = _lib.load()
        depth, intr = _f32c(depth, "depth"), _f32c(intr, "intr")
        m = _f32c(mask.float(), "mask")
        B, _, H, W = depth.shape
        Ho, Wo = H // dsp, W // dsp
        dev = depth.device
        seen = torch.empty(B, H * W, 3, dtype=torch.float32, device=dev)
        mean = torch.empty(B, 3, dtype=torch.float32, device=dev)
        scale = torch.empty(B, dtype=torch.float32, device=dev)
        coord = torch.empty(B, 3, Ho, Wo, dtype=torch.float32, device=dev)
        mask_dsp = torch.empty(B, 1, Ho, Wo, dtype=torch.float32, device=dev)
        with _lib.on(dev):
            _lib.check(lib.zs_seen_surface(_lib.ptr(depth), _lib.ptr(intr), _lib.ptr(m), B, H, W, Ho, Wo, _lib.ptr(seen),
                                           _lib.ptr(mean), _lib.ptr(scale), _lib.ptr(coord), _lib.ptr(mask_dsp),
                                           _stream(depth)), "zs_seen_surface")
        ctx.dsp = dsp
        ctx.save_for_backward(depth, intr, m, mean, scale, mask_dsp if dsp == 2 else None)
        ctx.mark_non_differentiable(mask_dsp)
        return seen, coord, mask_dsp

    @staticmethod
    def backward(ctx, d_seen, d_coord, _d_mask):
        lib = _lib.load()
        depth, intr, m, mean, scale, mask_dsp = ctx.saved_tensors
        B, _, H, W = depth.shape
        d_seen = None if d_seen is None else _f32c(d_seen, "seen grad")
        d_coord = None if d_coord is None else _f32c(d_coord, "coord grad")
        with _lib.on(depth.device):
            if ctx.dsp == 2 and d_coord is not None:      # the half-size map's gradient back at full size first
                d_full = torch.empty(B, 3, H, W, dtype=torch.float32, device=depth.device)
                _lib.check(lib.zs_coord_dsp2_bwd(_lib.ptr(d_coord), _lib.ptr(m), _lib.ptr(mask_dsp), _lib.ptr(d_full),
                                                 B, H, W, _stream(depth)), "zs_coord_dsp2_bwd")
                d_coord = d_full
            dd = torch.empty_like(depth)
            dk = torch.empty_like(intr)
            _lib.check(lib.zs_seen_surface_bwd(_lib.ptr(depth), _lib.ptr(intr), _lib.ptr(m), _lib.ptr(mean),
                                               _lib.ptr(scale), _lib.ptr(d_seen), _lib.ptr(d_coord), B, H, W,
                                               _lib.ptr(dd), _lib.ptr(dk), _stream(depth)), "zs_seen_surface_bwd")
        return dd, dk, None, None


def seen_surface(depth, intr, mask):
    return _SeenSurface.apply(depth, intr, mask, 1)


def seen_surface_dsp2(depth, intr, mask):
    return _SeenSurface.apply(depth, intr, mask, 2)


class _IntrParam2Mtx(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, H, W):
        lib = _lib.load()
        params = _f32c(params, "intr params")
        B = params.shape[0]
        intr = torch.empty(B, 3, 3, dtype=torch.float32, device=params.device)
        with _lib.on(params.device):
            _lib.check(lib.zs_intr_param2mtx(_lib.ptr(params), B, H, W, _lib.ptr(intr), _stream(params)),
                       "zs_intr_param2mtx")
        ctx.hw = (H, W)
        ctx.save_for_backward(params)
        return intr

    @staticmethod
    def backward(ctx, d_intr):
        lib = _lib.load()
        (params,) = ctx.saved_tensors
        d_intr = _f32c(d_intr, "intr grad")
        dp = torch.empty_like(params)
        with _lib.on(params.device):
            _lib.check(lib.zs_intr_param2mtx_bwd(_lib.ptr(params), _lib.ptr(d_intr), params.shape[0], ctx.hw[0],
                                                 ctx.hw[1], _lib.ptr(dp), _stream(params)), "zs_intr_param2mtx_bwd")
        return dp, None, None


def intr_param2mtx(params, H, W):
    return _IntrParam2Mtx.apply(params, H, W)


# ---- ViT token plumbing of DPT-hybrid (model/depth/vit.py:103-148, :31-43) ----
class _ResizeGrid(torch.autograd.Function):
    """Bilinear (align_corners=False) resize of a channels-last grid [Hi,Wi,C] -> [Ho,Wo,C]."""

    @staticmethod
    def forward(ctx, x, Ho, Wo):
        lib = _lib.load()
        x = _f32c(x, "resize input")
        Hi, Wi, C = x.shape
        y = torch.empty(Ho, Wo, C, dtype=torch.float32, device=x.device)
        with _lib.on(x.device):
            _lib.check(lib.zs_resize_bilinear_nhwc(_lib.ptr(x), _lib.ptr(y), Hi, Wi, Ho, Wo, C, 0, _stream(x)),
                       "zs_resize_bilinear_nhwc")
        ctx.shape = (Hi, Wi, Ho, Wo, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        Hi, Wi, Ho, Wo, C = ctx.shape
        dy = _f32c(dy, "resize grad")
        dx = torch.empty(Hi, Wi, C, dtype=torch.float32, device=dy.device)
        with _lib.on(dy.device):
            _lib.check(lib.zs_resize_bilinear_nhwc(_lib.ptr(dy), _lib.ptr(dx), Hi, Wi, Ho, Wo, C, 1, _stream(dy)),
                       "zs_resize_bilinear_nhwc(bwd)")
        return dx, None, None


def resize_grid(x, Ho, Wo):
    return _ResizeGrid.apply(x, Ho, Wo)


class _AssembleTokens(torch.autograd.Function):
    """tokens[b] = [cls | feat[b]] + pos   (feat [B,n,C], cls [C], pos [n+1,C])."""

    @staticmethod
    def forward(ctx, feat, cls, pos):
        return ops.assemble_tokens(_f32c(feat, "tokens"), _f32c(cls, "cls"), _f32c(pos, "pos"))

    @staticmethod
    def backward(ctx, dy):
        dy = _f32c(dy, "tokens grad")
        B, n1, C = dy.shape
        dpos = column_sum(dy.view(B, n1 * C)).view(n1, C)
        return dy[:, 1:].contiguous(), dpos[0].contiguous(), dpos


def assemble_tokens(feat, cls, pos):
    return _AssembleTokens.apply(feat, cls, pos)


class _WindowTokens(torch.autograd.Function):
    """CoordEmb's token preparation (seen_coord_enc.py:50-71; zs_window_tokens): emb [B,H,W,C], mask [B,H,W] bool,
    invalid_token [C], cls [C], pos [win*win+1, C] (fixed) -> [B*(H/win)*(W/win), win*win+1, C]."""

    @staticmethod
    def forward(ctx, emb, mask, invalid_token, cls, pos, win):
        emb, invalid_token = _f32c(emb, "window_tokens input"), _f32c(invalid_token, "invalid_coord_token")
        cls, pos = _f32c(cls, "cls_token"), _f32c(pos, "two_d_pos_embed")
        m = mask.to(torch.uint8).contiguous()      # converted here, once: the backward saves it, ops.window_tokens takes it as is
        ctx.save_for_backward(m)
        ctx.geom = tuple(emb.shape) + (win,)
        return ops.window_tokens(emb, m, invalid_token, cls, pos, win)

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (m,) = ctx.saved_tensors
        B, H, W, C, win = ctx.geom
        dy = _f32c(dy, "window_tokens grad")
        d_emb = torch.empty(B, H, W, C, dtype=torch.float32, device=dy.device)
        d_inv = torch.empty_like(d_emb)
        d_cls = torch.empty(B * (H // win) * (W // win), C, dtype=torch.float32, device=dy.device)
        with _lib.on(dy.device):
            _lib.check(lib.zs_window_tokens_bwd(_lib.ptr(dy), _lib.ptr(m), _lib.ptr(d_emb), _lib.ptr(d_inv), _lib.ptr(d_cls),
                                                B, H, W, C, win, _stream(dy)), "zs_window_tokens_bwd")
        return d_emb, None, column_sum(d_inv.view(-1, C)), column_sum(d_cls), None, None


def window_tokens(emb, mask, invalid_token, cls, pos, win):
    return _WindowTokens.apply(emb, mask, invalid_token, cls, pos, win)


class _ReadoutConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens):
        return ops.readout_concat(_f32c(tokens, "readout input"))

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        dy = _f32c(dy, "readout grad")
        B, n, C2 = dy.shape
        dt = torch.empty(B, n + 1, C2 // 2, dtype=torch.float32, device=dy.device)
        with _lib.on(dy.device):
            _lib.check(lib.zs_readout_concat_bwd(_lib.ptr(dy), _lib.ptr(dt), B, n, C2 // 2, _stream(dy)),
                       "zs_readout_concat_bwd")
        return dt


def readout_concat(tokens):
    return _ReadoutConcat.apply(tokens)


# ---- the depth task's losses (options/depth.yaml) ----
class _MidasLoss(torch.autograd.Function):
    """MidasLoss.forward (model/depth/midas_loss.py:166-185): ssi MAE + alpha * gradient matching."""

    @staticmethod
    def forward(ctx, prediction, target, mask, alpha, scales, inverse_depth):
        lib = _lib.load()
        p, t = _f32c(prediction, "depth prediction"), _f32c(target.float(), "depth target")
        m = _f32c(mask.float(), "depth mask")
        B, _, H, W = p.shape
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        ws = torch.empty((_ws_bytes("zs_midas_loss_workspace_bytes", B) + 3) // 4, dtype=torch.float32, device=p.device)
        with _lib.on(p.device):
            _lib.check(lib.zs_midas_loss(_lib.ptr(p), _lib.ptr(t), _lib.ptr(m), B, H, W, float(alpha), int(scales),
                                         1 if inverse_depth else 0, _lib.ptr(loss), _lib.ptr(ws), _stream(p)),
                       "zs_midas_loss")
        ctx.cfg = (alpha, scales, inverse_depth)
        ctx.save_for_backward(p, t, m, ws)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        p, t, m, ws = ctx.saved_tensors
        alpha, scales, inverse_depth = ctx.cfg
        B, _, H, W = p.shape
        dloss = _f32c(dloss, "loss grad")
        dp = torch.empty_like(p)
        with _lib.on(p.device):
            _lib.check(lib.zs_midas_loss_bwd(_lib.ptr(p), _lib.ptr(t), _lib.ptr(m), B, H, W, float(alpha), int(scales),
                                             1 if inverse_depth else 0, _lib.ptr(ws), _lib.ptr(dloss), _lib.ptr(dp),
                                             _stream(p)), "zs_midas_loss_bwd")
        return dp, None, None, None, None, None


@torch.no_grad()
def erode_mask(mask, pool=4):
    """MidasLoss.erode_mask (model/depth/midas_loss.py:153-162): [B,1,H,W] -> [B,1,H,W] in {0, 1}."""
    lib = _lib.load()
    m = _f32c(mask.float(), "mask")
    B, _, H, W = m.shape
    out = torch.empty_like(m)
    with _lib.on(m.device):
        _lib.check(lib.zs_erode_mask(_lib.ptr(m), B, H, W, pool, _lib.ptr(out), _stream(m)), "zs_erode_mask")
    return out


def midas_loss(prediction, target, mask, alpha=0.1, scales=4, inverse_depth=True):
    return _MidasLoss.apply(prediction, target, mask, alpha, scales, inverse_depth)


class _IntrLoss(torch.autograd.Function):
    """Loss.intr_loss (utils/loss.py:36-43)."""

    @staticmethod
    def forward(ctx, seen_pred, seen_gt, mask):
        lib = _lib.load()
        a, b, m = _f32c(seen_pred, "seen_pred"), _f32c(seen_gt.float(), "seen_gt"), _f32c(mask.float(), "mask")
        n = m.numel()
        assert a.numel() == 3 * n and b.numel() == 3 * n
        out = torch.empty(2, dtype=torch.float32, device=a.device)
        with _lib.on(a.device):
            _lib.check(lib.zs_intr_loss(_lib.ptr(a), _lib.ptr(b), _lib.ptr(m), n, _lib.ptr(out), _stream(a)), "zs_intr_loss")
        ctx.save_for_backward(a, b, m, out)
        return out[0].clone()

    @staticmethod
    def backward(ctx, dloss):
        lib = _lib.load()
        a, b, m, out = ctx.saved_tensors
        dloss = _f32c(dloss, "loss grad")
        da = torch.empty_like(a)
        with _lib.on(a.device):
            _lib.check(lib.zs_intr_loss_bwd(_lib.ptr(a), _lib.ptr(b), _lib.ptr(m), m.numel(), _lib.ptr(out), _lib.ptr(dloss),
                                            _lib.ptr(da), _stream(a)), "zs_intr_loss_bwd")
        return da, None, None


def intr_loss(seen_pred, seen_gt, mask):
    return _IntrLoss.apply(seen_pred, seen_gt, mask)
