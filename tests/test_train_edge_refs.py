"""CPU side of tests/test_gpu_train_edges.py: the evidence that its references and inputs are sound.

 - the float64 restatement of the seen-surface geometry agrees with oracle/frontend_ref on the inputs of section D;
 - every "measured" tolerance of the GPU module is at least 4 x the error of fp32 CPU torch (or of the fp32 oracle)
   against the float64 reference on the same input, recomputed here;
 - every masked input keeps the float64 reference finite (no 0 / 0 sample, no entry compared against zero)."""
import pytest
import torch

from oracle import frontend_ref, train_ref
from tests import test_gpu_train_edges as E
from tests.test_gpu_train_ops import close

F32 = torch.float32
ONE_PIXEL_LOSS = 1.865290021622           # oracle/loss_ref.midas_loss in float64 on midas_one_valid_pixel()


def noise(ref_fn, *args):
    lo, hi = ref_fn(*args, dtype=F32), ref_fn(*args, dtype=E.F64)
    return {k: E.relerr(lo[k], hi[k]) for k in hi}


def pinned(what, errs, tol):
    print("%s: fp32 torch against float64: %s" % (what, " ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    for k, e in errs.items():
        assert 4 * e <= tol[k], "%s %s: 4 x %.3e above the tolerance %.3e" % (what, k, e, tol[k])


@pytest.mark.parametrize("crop", E.SEEN_CROPS, ids=lambda c: "%dx%d_dsp%d" % c[2:])
def test_float64_seen_surface_agrees_with_the_oracle(crop):
    inp = E.seen_inputs(crop)
    H, W = inp["depth"].shape[2:]
    close(E.intr_param2mtx_ref(H, W, inp["params"]), frontend_ref.intr_param2mtx(H, W, inp["params"]), rtol=1e-6, what="intr")
    want = frontend_ref.seen_surface(inp["depth"], inp["K"], inp["mask"], inp["dsp"])
    with torch.no_grad():
        got = E.seen_surface_ref(inp["depth"].double(), inp["K"].double(), inp["mask"].double(), inp["dsp"])
    for name, g, w in zip(("seen", "coord", "mask", "mean", "scale"), got, want):
        assert bool(torch.isfinite(g).all()), name
        if name == "mask":
            assert torch.equal(g.float(), w)
        else:
            close(w, g, rtol=E.SEEN_VAL, what=name)                 # the fp32 oracle against float64


def test_ill_conditioned_tolerances_cover_fp32_noise():
    pinned("layer_norm", noise(E.ln_reference, E.ln_inputs(*E.LN_ILL_CASE, ill=True), True), E.LN_ILL_TOL)
    shape, relu, res = E.BN_ILL_CASE
    pinned("batch_norm", noise(E.bn_reference, E.bn_inputs(shape, res, ill=True), relu), E.BN_ILL_TOL)
    cfg, relu, res = E.GN_ILL_CASE
    pinned("group_norm", noise(E.gn_reference, E.gn_inputs(cfg, res, ill=True), relu), E.GN_ILL_TOL)


def test_two_pass_group_norm_is_group_norm():
    for cfg, relu, res in E.GN_CASES[:4] + [E.GN_ILL_CASE]:
        inp = E.gn_inputs(cfg, res, ill=cfg == E.GN_ILL_CASE[0])
        x = inp["x"].double()
        want = torch.nn.functional.group_norm(x.permute(0, 3, 1, 2), inp["groups"], inp["gamma"].double(), inp["beta"].double(),
                                              1e-5).permute(0, 2, 3, 1)
        close(E.group_norm_two_pass(x, inp["groups"], inp["gamma"].double(), inp["beta"].double(), 1e-5), want, rtol=1e-9,
              what="group_norm %s" % (cfg,))


def test_large_logit_tolerances_cover_fp32_noise():
    for c in E.ATT_BIG_CASES:
        pinned("attention x4 %s" % (c,), noise(E.attention_reference, E.attention_inputs(*c, mult=4.0)), E.ATT_BIG_TOL)
    pinned("point attention x4", noise(E.point_attention_reference, E.point_attention_inputs(*E.PA_NUMERIC_CASE, mult=4.0)),
           E.PA_BIG_TOL)
    pinned("point attention self", noise(E.point_attention_reference,
                                         E.point_attention_inputs(*E.PA_NUMERIC_CASE, self_dominant=True)), E.PA_TOL)


@pytest.mark.parametrize("crop", E.SEEN_CROPS, ids=lambda c: "%dx%d_dsp%d" % c[2:])
def test_d_intr_entry_tolerance_covers_the_fp32_oracle(crop):
    inp = E.seen_inputs(crop)
    want = E.seen_reference(inp)
    assert float(want["d_leaf"].abs().min()) > 0                   # every entry is compared against itself
    for use in (("seen", "coord"), ("seen",), ("coord",)):
        want = E.seen_reference(inp, use)
        d, K = inp["depth"].clone().requires_grad_(True), inp["K"].clone().requires_grad_(True)
        with train_ref.differentiable():
            seen, coord = frontend_ref.seen_surface(d, K, inp["mask"], inp["dsp"])[:2]
            loss = (seen * inp["gs"]).sum() if "seen" in use else 0
            (loss + ((coord * inp["gc"]).sum() if "coord" in use else 0)).backward()
        err = E.entry_errors(K.grad, want["d_leaf"])
        print("fp32 oracle d_intr entry errors %s %s: %s" % (crop, use, " ".join("%.2e" % e for e in err.tolist())))
        assert 4 * float(err.max()) <= E.D_INTR_ENTRY_TOL
        close(d.grad, want["d_depth"], rtol=E.SEEN_GRAD, what="d_depth")


def _torch_norm_noise(grads):
    ps = [torch.zeros_like(gr).requires_grad_(True) for gr in grads]
    for p, gr in zip(ps, grads):
        p.grad = gr.clone()
    want = E.norm64(grads)
    return abs(float(torch.nn.utils.clip_grad_norm_(ps, 1e9)) - want) / want


def test_grad_norm_tolerance_covers_fp32_torch():
    """Every norm the GPU module asserts: the edge-weighted gradients together and tensor by tensor, and the five draws
    of the clipping tests."""
    init, grads = E.grad_norm_inputs()
    worst = max([_torch_norm_noise(grads)] + [_torch_norm_noise([gr]) for gr in grads])
    g, _ = E.clip_params()
    draws = [E.clip_grads(g) for _ in range(5)]
    worst = max([worst] + [_torch_norm_noise(d) for d in draws])
    print("grad norm: fp32 torch against float64, worst of all cases %.2e" % worst)
    assert 4 * worst <= E.GRAD_NORM_TOL <= 4.1 * worst             # the rule's value, not a looser one
    # a lost tail chunk, last element or one-element tensor moves the norm by far more than the tolerance
    want = E.norm64(grads)
    for (t, e) in E.GRAD_NORM_EDGES:
        cut = [gr.clone() for gr in grads]
        cut[t].view(-1)[e] = 0
        assert abs(E.norm64(cut) - want) > 1000 * E.GRAD_NORM_TOL * want, (t, e)
        assert abs(E.norm64([cut[t]]) - E.norm64([grads[t]])) > 1000 * E.GRAD_NORM_TOL * E.norm64([grads[t]]), (t, e)
    assert all(E.norm64(d) > max(E.CLIP_BELOW) for d in draws)      # the "below" run clips on every step
    assert len({round(c / E.norm64(d), 6) for c, d in zip(E.CLIP_BELOW, draws)}) == 4    # by a different factor each


def test_masked_inputs_keep_the_references_finite():
    for inv in (True, False):
        for shape in E.MIDAS_SHAPES:
            inp = E.midas_inputs(*shape, inv)
            assert int(inp["mask"].sum((1, 2, 3)).min()) >= 4
            assert bool((inp["pred"] < 0).any()) == (not inv)
            loss, grad = E.midas_reference(inp)
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
            lo, glo = E.midas_reference(inp, dtype=F32)             # the fp32 oracle sits well inside the tolerances
            assert abs(float(lo) - float(loss)) <= E.MIDAS_LOSS / 4 * abs(float(loss)), (shape, inv)
            assert E.relerr(glo, grad) <= E.MIDAS_GRAD / 4, (shape, inv, E.relerr(glo, grad))
    inp = E.midas_one_valid_pixel()
    assert int(inp["mask"][0].sum()) == 1 and int(inp["mask"][1].sum()) >= 4
    loss, grad = E.midas_reference(inp)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert float(grad[0].abs().max()) == 0 and float(grad[1].abs().max()) > 0
    assert abs(float(loss) - ONE_PIXEL_LOSS) < 1e-9, float(loss)   # freezes the det == 0 branch of the oracle
    inp = E.midas_one_sample_masked()
    assert int(inp["mask"][1].sum()) == 0 and int(inp["mask"][[0, 2]].sum((1, 2, 3)).min()) >= 4
    loss, grad = E.midas_reference(inp)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()) and float(grad[1].abs().max()) == 0
    for crop in E.SEEN_CROPS:
        inp = E.seen_inputs(crop)
        assert int(inp["mask"].sum((1, 2, 3)).min()) >= 113
        for use in (("seen", "coord"), ("seen",), ("coord",)):
            want = E.seen_reference(inp, use)
            assert all(bool(torch.isfinite(v).all()) for v in want.values())
            assert float(want["d_leaf"].abs().min()) > 0
        assert bool(torch.isfinite(E.seen_reference(E.seen_inputs(crop, full_matrix=False), chained=True)["d_leaf"]).all())
