"""GPU tests of the fp6 MX operand and its products (include/lq_hip.h: lq_mx6_*).  Pack and quantize are held BYTE FOR BYTE to the
NumPy packer of the documented layout; the lane map of 6-bit data is pinned by a one-term sweep over every k and by exact products
of all 16 pairs with an fp6 side, BIT FOR BIT against float64; random data is held to the project's 1e-5 * sum|terms|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mx6_reference as R
import _mx_conv_reference as C
import _mx_gemm_reference as G
from _arena import Arena
from _bounds import REL, assert_within_terms

import learned_quantization_amd as lq
from learned_quantization_amd import _hip, layers as L, ops

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
_ids = lambda d: "-".join(map(str, d)) if isinstance(d, tuple) else str(d)      # noqa: E731
_t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
f64 = lambda a: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)      # noqa: E731
_pack = lambda P, s, name: (ops.mx6_operand_pack if name in R.FORMATS6 else ops.mx_operand_pack)(_t(P), _t(s), name)      # noqa: E731
_quantize = lambda x, name, m="mx": (ops.mx6_operand_quantize if name in R.FORMATS6 else ops.mx_operand_quantize)(_t(x), name, m)      # noqa: E731
_exact = {shape: G.exact_case(*shape) for shape in [(16, 16, 160), (16, 16, 128), (19, 21, 160), (37, 10, 784)]}


def _assert_layout(op, ref):
    (wc, ws), gc, gs = R.pack_layout(ref.codes, ref.bytes), op.codes.cpu().numpy(), op.scales.cpu().numpy()
    assert isinstance(op, ops.Mx6Operand) and (op.lines, op.K) == ref.codes.shape
    assert (op.codes.numel(), op.scales.numel()) == ops.mx6_operand_bytes(op.format, op.lines, op.K) == (wc.size, ws.size)
    assert np.array_equal(gc, wc) and np.array_equal(gs, ws), f"{int((gc != wc).sum())} code and {int((gs != ws).sum())} scale bytes differ"


@pytest.mark.parametrize("case", G.PACK_SHAPES + [(m, *s) for m in ("mx", "cover") for s in G.QUANT_SHAPES], ids=_ids)
@pytest.mark.parametrize("name", R.FORMATS6)
def test_pack_and_quantize_write_the_documented_layout(name, case):
    """Pack (R, C, axis), whose decode is fq_forward_mx's ``out`` bit for bit; quantize (method, M, K)."""
    if isinstance(case[0], str):
        x = G.quantize_case(*case[1:])
        return _assert_layout(_quantize(x, name, case[0]), G.operand_of_activation(x, name, case[0])[0])
    P, s = G.pack_case("gauss", name, *case)
    op = _pack(P, s, name)
    _assert_layout(op, G.operand_of_parameter(P, s, name, case[2]))
    out = ops.fq_forward_mx(_t(P), _t(s), name, 32, "e8m0")
    assert torch.equal(ops.mx_operand_decode(op).view(torch.int32), (out.T.contiguous() if case[2] == 0 else out).view(torch.int32))


@pytest.mark.parametrize("name", R.FORMATS6)
@pytest.mark.parametrize("side", ["A", "B"])
def test_map_sweep_one_term_per_output(side, name):
    """16 x 16 x 160: two K steps, the second ragged.  A holds ONE non-zero element, at k, for every k in turn; B differs by k and by
    line, the scale bytes by block: Y must be that single product.  The fp6 operand is A (``side`` A) or B."""
    c, (fa, fb) = _exact[(16, 16, 160)], (name, "fp8_e4m3") if side == "A" else ("fp8_e4m3", name)
    b = _pack(c["W"], c["sw"], fb)
    for k in range(160):
        m, A = (5 * k + 3) % 16, np.zeros((16, 160), np.float32)
        A[m, k] = -1.5 * c["sa"][m, k // 32]
        Y, ref = f64(ops.mx_gemm(_pack(A, c["sa"], fa), b)), f64(A) @ f64(c["W"])
        assert np.array_equal(Y, ref), f"k = {k}: first wrong (m, n) = {tuple(np.argwhere(Y != ref)[0])}"


@pytest.mark.parametrize("shape", [(16, 16, 128), (19, 21, 160), (37, 10, 784)], ids=_ids)
@pytest.mark.parametrize("pair", R.PAIRS, ids=_ids)
def test_gemm_exact_is_the_float64_product_bit_for_bit(pair, shape):
    """Every partial sum is a float32 (tests/test_mx_gemm_cpu.py).  K = 160 runs with a bias, K = 784 into ``out=`` with a row stride."""
    (M, N, K), c = shape, _exact[shape]
    a, b = _pack(c["A"], c["sa"], pair[0]), _pack(c["W"], c["sw"], pair[1])
    bias, buf = c["bias"] if K == 160 else None, torch.full((M, N + 3), -7.0, device=dev)
    Y = ops.mx_gemm(a, b, None if bias is None else _t(bias), out=buf[:, :N] if K == 784 else None)
    bad = np.argwhere(f64(Y) != f64(c["A"]) @ f64(c["W"]) + (0.0 if bias is None else f64(bias)))
    assert bad.size == 0, f"{len(bad)} of {M * N} outputs differ, first at (m, n) = {tuple(bad[0])}"
    assert (buf[:, N:] == -7.0).all() and (K != 784 or Y.data_ptr() == buf.data_ptr())


@pytest.mark.parametrize("pair", R.PAIRS, ids=_ids)
def test_gemm_random_within_the_yardstick(pair):
    c = G.random_case(81, 70, 160, *pair)
    a, b, bias = _quantize(c["x"], pair[0]), _pack(c["W"], c["sw"], pair[1]), f64(c["bias"])[None, :]
    Y, A, B = ops.mx_gemm(a, b, _t(c["bias"])), f64(ops.mx_operand_decode(a)), f64(ops.mx_operand_decode(b))
    ref, terms = A @ B.T + bias, np.abs(A) @ np.abs(B).T + np.abs(bias)
    print(f"mx6_gemm {pair[0]} x {pair[1]}: worst err / sum|terms| = {float((np.abs(f64(Y) - ref) / terms).max()):.3e} (REL = {REL:g})")
    assert_within_terms(f64(Y), ref, terms, f"mx6_gemm {pair}")


@pytest.mark.parametrize("shape", [(17, 33, 160), (81, 70, 160)], ids=_ids)
@pytest.mark.parametrize("out_format", ["fp8_e4m3", "fp4_e2m1"])
@pytest.mark.parametrize("activation", [None, "relu"])
@pytest.mark.parametrize("pair", [("fp8_e4m3", "fp6_e2m3"), ("fp6_e3m2", "fp4_e2m1")], ids=_ids)
def test_epilogue_is_the_composition_byte_for_byte(pair, activation, out_format, shape):
    c = G.random_case(*shape, *pair)
    a, b, bias = _quantize(c["x"], pair[0]), _pack(c["W"], c["sw"], pair[1]), _t(c["bias"])
    got, y = ops.mx_gemm_quantize(a, b, bias, activation, out_format, "mx"), ops.mx_gemm(a, b, bias)
    want = ops.mx_operand_quantize(torch.relu(y) if activation else y, out_format, "mx")
    assert isinstance(got, ops.MxOperand) and got[2:] == want[2:] and torch.equal(got.codes, want.codes) and torch.equal(got.scales, want.scales)


def test_capture_replay_between_guard_bands():
    """One launch each in one graph.  The outputs lie between tests/_arena.py's guard bands at their exact sizes, reset before each replay."""
    M, N, K, fa, fb = 19, 21, 160, "fp6_e2m3", "fp6_e3m2"
    c = {key: _t(v) for key, v in G.random_case(M, N, K, fa, fb).items()}
    ea, eb = ops.mx6_operand_quantize(c["x"], fa), ops.mx6_operand_pack(c["W"], c["sw"], fb)
    eager = dict(bc=eb.codes, bs=eb.scales, ac=ea.codes, as_=ea.scales, Y=ops.mx_gemm(ea, eb, c["bias"]).view(torch.uint8).reshape(-1))
    ar = Arena(dev)
    for key, t in eager.items():                           # scales are "some": a padding dword of bytes 127 IS the sentinel word
        ar.add(key, "some" if key in ("as_", "bs") else "out", nbytes=t.numel())
    ar.build()
    lib, p, (x, W, sw, bias) = _hip.load(), ar.ptr, (c[key].data_ptr() for key in ("x", "W", "sw", "bias"))
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # element formats 1 and 2: LQ_ELEM_FP6_E2M3, LQ_ELEM_FP6_E3M2
        st = _hip.stream_ptr(dev)
        _hip.check(lib.lq_mx6_operand_pack(W, sw, 2, 0, K, N, 0, 32, p("bc"), p("bs"), st), "pack")
        _hip.check(lib.lq_mx6_operand_quantize(x, 1, 0, M, K, p("ac"), p("as_"), st), "quantize")
        _hip.check(lib.lq_mx6_gemm(p("ac"), p("as_"), 1, p("bc"), p("bs"), 2, bias, p("Y"), M, N, K, N, st), "gemm")
    for _ in range(2):
        ar.buf.fill_(0x7F)
        g.replay()
        torch.cuda.synchronize(dev)
        ar.check("mx6 pack, quantize and gemm")
        assert all(torch.equal(ar.bytes(key), t) for key, t in eager.items()), "a replayed buffer differs from the eager call"


@pytest.mark.parametrize("kind", ["dense", "conv"])
def test_layers_call_mx_fp6(kind):
    """Exact data against float64 matmul / F.conv2d ('SAME' pads top 1, bottom 1, right 1) bit for bit; random data against emulate=True."""
    kw = dict(orientation="groupwise", element_format="fp6_e2m3", device=dev)
    if kind == "dense":
        c, quantize = _exact[(19, 21, 160)], ops.mx_operand_quantize
        layer = lq.CustomDenseLayer(units=21, input_shape=160, trained_weights=[c["W"], c["bias"]], **kw)
        layer.nested_q_w_layer.scale.data.copy_(_t(c["sw"]))
        x, ref = c["A"], f64(c["A"]) @ f64(c["W"]) + f64(c["bias"])
    else:
        g, quantize = C.Geom(2, 5, 9, 10, 3, 3, 2, 2, "SAME"), lambda t: ops.mx_operand_im2col(t, (3, 3), (2, 2), (1, 1, 0, 1))
        (k, bias), x = C.exact_kernel(g, 24), C.exact_input(g)
        layer = lq.CustomConv2DLayer(filters=24, kernel_size=(3, 3), strides=(2, 2), padding="same", input_shape=g.C, data_format="NCHW",
                                     trained_weights=[k, bias], **kw)
        layer.nested_q_k_layer.scale.data.fill_(1.0)
        k64, b64, x64 = (torch.from_numpy(f64(v)) for v in (k.transpose(3, 2, 0, 1), bias, x))
        ref = F.conv2d(F.pad(x64, (0, 1, 1, 1)), k64, b64, (2, 2)).numpy()
    layer.nested_q_b_layer.scale.data.fill_(1.0)           # the bias is on the e2m3 grid under scale 1
    w6 =layer.eval().mx_operand(fp6=True)
    for act_format in ("fp8_e4m3", "fp4_e2m1"):
        assert isinstance(w6, ops.Mx6Operand) and np.array_equal(f64(layer.call_mx(_t(x), act_format, fp6=True)), ref), act_format
    xr = torch.randn(x.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    with L.mx_hardware(layer, emulate=True, convs=True, fp6=True) as hw, torch.no_grad():
        assert hw.layers == [layer]
        emu = layer(xr)
    terms = np.abs(f64(ops.mx_operand_decode(quantize(xr)))) @ np.abs(f64(ops.mx_operand_decode(w6))).T + np.abs(f64(layer.b))
    assert_within_terms(f64(layer.call_mx(xr, fp6=True).movedim(1, -1)), f64(emu.movedim(1, -1)), terms, f"{kind} call_mx against emulate=True")


def test_mx_hardware_fp6_on_the_mnist_model():
    model = lq.build_model("mnist", mode="ste", value=0.0, seed=3, device=dev, element_format="fp6_e2m3", scale_init="cover").eval()
    x = torch.rand(37, 1, 28, 28, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    with torch.no_grad():
        before = model(x)
        with L.mx_hardware(model) as hw:                   # without the opt-in nothing switches
            assert hw.layers == [] and torch.equal(model(x), before)
        with L.mx_hardware(model, fp6=True) as hw:
            assert hw.layers == [model.dense_1, model.dense_2] and all(isinstance(m._mx_hw[0], ops.Mx6Operand) for m in hw.layers)
            unfused = model(x)
        with L.mx_hardware(model, fp6=True, fused=True) as hw:
            assert hw.fused_layers == [model.dense_1, model.dense_2]
            assert torch.equal(model(x).view(torch.int32), unfused.view(torch.int32)) and not torch.equal(unfused, before)
