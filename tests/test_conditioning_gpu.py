"""Every kernel family on ill-conditioned inputs (tests/conditioning.py) against the fp64 oracles, and power-of-two
homogeneity of every backward.

The recipes, the update-wise / region-wise comparison and the fairness condition (the fp32 oracle on the CPU stays within 0.25
of util.FWD / util.BWD on every pair run here: tests/test_conditioning_cpu.py) are described in conditioning.py.  Tolerances
are util.FWD / util.BWD, unchanged.  EGT_CONDITIONING_MARGINS=<file> additionally writes the worst measured margin per
(operator, recipe) to that file (profiles/conditioning_margins.json is such a dump)."""
import ctypes as C
import json
import os

import pytest
import torch

import conditioning as CD

pytestmark = pytest.mark.gpu

MARGINS = {}     # operator -> recipe -> [worst margin, "case / output"]

# (operator, case id, recipe) -> reason with the measured margin: strict expected failures, listed under the gaps of DESIGN.md
_FFN_ELU = ("ffn_act (csrc/egt_ffn.hip) takes ELU as the fast exp minus 1: 6e-8 absolute on hidden values of ~1e-4; margin {} on "
            "d lr2_kernel.  Both accurate forms cost more than the parent's spread of the layers-scope step (DESIGN.md, gaps)")
XFAIL = {
    ("ffn", "W64_f32_fp32_elu", "small_weights4"): _FFN_ELU.format("1.118"),
    ("ffn", "W64_bf16x3_fp32_elu", "small_weights4"): _FFN_ELU.format("1.093"),
}


def _p(op, cid, recipe, *values):
    why = XFAIL.get((op, cid, recipe))
    return pytest.param(*values, id=f"{cid}-{recipe}", marks=[pytest.mark.xfail(strict=True, reason=why)] if why else [])


@pytest.fixture(scope="module", autouse=True)
def _dump_margins():
    yield
    path = os.environ.get("EGT_CONDITIONING_MARGINS")
    if path and MARGINS:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(tolerance="util.FWD / util.BWD (the bf16 two-layer stack case: util.bf16_stack_tol(1) against the storage-aware "
                                     "oracle); margin = worst |error| / tolerance under conditioning.compare (< 1 passes)",
                           worst_margin={op: {r: dict(margin=round(v[0], 4), where=v[1]) for r, v in sorted(d.items())}
                                         for op, d in sorted(MARGINS.items())}), f, indent=1, sort_keys=True)


def _check(case, got, ref):
    sink = {}
    try:
        CD.compare(got, ref, case, check=False, sink=sink)          # measure first: a failing case still reports its margin
    finally:
        slot = MARGINS.setdefault(case["op"], {})
        for name, m in sink.items():
            if m > slot.get(case["recipe"], [-1.0])[0]:
                slot[case["recipe"]] = [m, f"{case['id']} / {name}"]
    if sink:
        top = max(sink, key=sink.get)
        print(f"[conditioning] {case['op']} {case['id']} {case['recipe']}: worst margin {sink[top]:.3f} on {top}")
    CD.compare(got, ref, case)


# ------------------------------------------------------------------------------------------------------ fused block --
def _assert_family(case, mod, blocks, egt_lib):
    """the descriptor must reach the kernels the case is named after"""
    from egt_amd import fused as FZ
    c = case["c"]
    blk = blocks[0]
    if c["bwd"] is None:
        assert blk.last_path == "fused-pair", blk.last_path
        return
    static = c.get("ect") == "bias" and case["layers"] == 1
    desc = FZ._desc(blk, c["B"], c["N"], False, 0, torch.bfloat16 if c.get("bf16") else torch.float32, static_edge=static)
    assert egt_lib.egt_block_bwd_kernel(C.byref(desc)).decode() == c["bwd"]
    form = egt_lib.egt_block_launch_form(C.byref(desc)).decode()
    assert f"fwd={c['fwd']}/" in form and f"bwd={c['bwd']}/" in form, form
    if case["layers"] == 1:
        assert blk.last_path == "fused", blk.last_path
        if static:
            assert blk.last_edge_route == "static", blk.last_edge_route
    else:
        assert mod.last_path == "fused-stack", mod.last_path


BLOCK_PARAMS = [_p("block" if layers == 1 else "stack", f"{cid}-L{layers}", recipe, cid, recipe, layers)
                for layers in (1, 2) for cid in CD.BLOCK_CASES for recipe in CD.BLOCK_RECIPES
                if not CD.excluded("block" if layers == 1 else "stack", cid, recipe)]


@pytest.mark.parametrize("cid,recipe,layers", BLOCK_PARAMS)
def test_block(cid, recipe, layers, gpu, egt_lib):
    """one EGTBlock(fused) call (layers = 1; the 'bias' case on the static-edge route) and one two-layer egt_stack_* call:
    forward, backward and all 14 parameter gradients per layer"""
    case = CD.make_block(cid, recipe, layers)
    got, mod, blocks = CD.block_gpu(case, gpu)
    _assert_family(case, mod, blocks, egt_lib)
    if case["c"].get("bf16"):
        assert got["e_out"].dtype == torch.bfloat16 and got["de"].dtype == torch.bfloat16
    _check(case, got, CD.block_oracle(case))


# --------------------------------------------------------------------------------------------------------- inner op --
@pytest.mark.parametrize("cid,recipe", [_p("attn", cid, recipe, cid, recipe) for cid in CD.ATTN_CASES for recipe in CD.ATTN_RECIPES])
def test_attention(cid, recipe, gpu, egt_lib):
    case = CD.make_attn(cid, recipe)
    _check(case, CD.attn_gpu(case, gpu), CD.attn_oracle(case))


# --------------------------------------------------------------------------------------------- edge_proj, edge_update --
@pytest.mark.parametrize("De,act,recipe", [_p("edge_proj", f"De{De}_{act}", recipe, De, act, recipe) for De, act in CD.EDGE_CASES
                                           for recipe in CD.edge_proj_recipes(act)])
def test_edge_proj(De, act, recipe, gpu, egt_lib):
    case = CD.make_edge_proj(De, act, recipe)
    _check(case, CD.edge_proj_gpu(case, gpu), CD.edge_proj_oracle(case))


@pytest.mark.parametrize("De,recipe", [_p("edge_update", f"De{De}", recipe, De, recipe) for De in (64, 8) for recipe in CD.EDGE_RECIPES])
def test_edge_update(De, recipe, gpu, egt_lib):
    case = CD.make_edge_update(De, recipe)
    _check(case, CD.edge_update_gpu(case, gpu), CD.edge_update_oracle(case))


# ------------------------------------------------------------------------------------------------------ channel FFN --
@pytest.mark.parametrize("W,matmul,bf16,act,recipe", [
    _p("ffn", f"W{W}_{mm}_{'bf16' if bf else 'fp32'}_{act}", recipe, W, mm, bf, act, recipe)
    for W, mm, bf, act in CD.FFN_CASES for recipe in CD.ffn_recipes(act)])
def test_ffn(W, matmul, bf16, act, recipe, gpu, egt_lib):
    case = CD.make_ffn(W, matmul, bf16, act, recipe)
    got = CD.ffn_gpu(case, gpu)
    if bf16:
        assert got["y"].dtype == torch.bfloat16 and got["dx"].dtype == torch.bfloat16
    _check(case, got, CD.ffn_oracle(case))


# --------------------------------------------------------------------------------------------------- cross-talk FFN --
@pytest.mark.parametrize("cid,recipe", [_p("xtalk", cid, recipe, cid, recipe) for cid in CD.XTALK_CASES for recipe in CD.xtalk_recipes(cid)])
def test_xtalk(cid, recipe, gpu, egt_lib):
    """the full xtalk_ffn (fused edge side, torch node side): h', e', dh, de and the twelve parameter gradients"""
    case = CD.make_xtalk(cid, recipe)
    _check(case, CD.xtalk_gpu(case, gpu), CD.xtalk_oracle(case))


# ------------------------------------------------------------------------------------------------------------ heads --
@pytest.mark.parametrize("case,recipe", [_p("edge_head", "-".join(map(str, c)), recipe, c, recipe) for c in CD.EDGE_HEAD_CASES
                                         for recipe in CD.HEAD_RECIPES])
def test_edge_head(case, recipe, gpu, egt_lib):
    c = CD.make_edge_head(*case, recipe)
    _check(c, CD.edge_head_gpu(c, gpu), CD.edge_head_oracle(c))


@pytest.mark.parametrize("case,recipe", [_p("node_head", "-".join(map(str, c)), recipe, c, recipe) for c in CD.NODE_HEAD_CASES
                                         for recipe in CD.NODE_HEAD_RECIPES])
def test_node_head(case, recipe, gpu, egt_lib):
    c = CD.make_node_head(*case, recipe)
    got, ref = CD.node_head_gpu(c, gpu), CD.node_head_oracle(c)
    _check(c, got, ref)
    assert float(got["counts"][1]) == float(ref["counts"][1]), "rows: exact"
    if ref["gap"] > 1e-3:          # (hits are exact where no two class logits tie within the forward tolerance)
        assert float(got["counts"][0]) == float(ref["counts"][0]), "hits: exact"


# ------------------------------------------------------------------------------------- power-of-two homogeneity --
# A backward is linear in its upstream gradient and a power of two scales exactly: backward(2^k dy) == 2^k backward(dy),
# bit for bit, for every output and parameter gradient.  Inputs stay unit-scale (recipe "plain"), so nothing leaves the
# normal range.  A difference means the kernel adds something that did not come from dy.
def _homogeneous(case, run, gpu):
    grads = [name for name, kind, _, _ in case["spec"] if kind == "bwd"]
    base = run(case, gpu)
    base = base[0] if isinstance(base, tuple) else base
    for k in (10, -10):
        f = 2.0 ** k
        out = run(CD.scaled_upstream(case, f), gpu)
        out = out[0] if isinstance(out, tuple) else out
        for name in grads:
            a, b = out.get(name), base.get(name)
            if b is None:
                assert a is None, name
                continue
            assert torch.equal(a.float(), b.float() * f), f"{name}: backward(2^{k} dy) != 2^{k} backward(dy)"


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("cid", list(CD.BLOCK_CASES))
def test_block_backward_is_homogeneous(cid, layers, gpu, egt_lib):
    """egt_block_bwd / egt_stack_bwd of every family (v4_de64_bf16: bf16 edge storage) and the pair operator"""
    _homogeneous(CD.make_block(cid, "plain", layers), CD.block_gpu, gpu)


@pytest.mark.parametrize("cid", list(CD.ATTN_CASES)[:4])
def test_attention_backward_is_homogeneous(cid, gpu, egt_lib):
    _homogeneous(CD.make_attn(cid, "plain"), CD.attn_gpu, gpu)


@pytest.mark.parametrize("De,act", [(64, None), (8, "elu"), (64, "lrelu2")])
def test_edge_backwards_are_homogeneous(De, act, gpu, egt_lib):
    _homogeneous(CD.make_edge_proj(De, act, "plain"), CD.edge_proj_gpu, gpu)
    _homogeneous(CD.make_edge_update(De, "plain"), CD.edge_update_gpu, gpu)


@pytest.mark.parametrize("W,matmul,bf16,act", [(64, "f32", False, "elu"), (64, "bf16x3", True, "elu"), (16, "f32", True, "relu"),
                                               (16, "bf16x3", False, "elu"), (8, "f32", False, "elu"), (8, "f32", True, "relu")])
def test_ffn_backward_is_homogeneous(W, matmul, bf16, act, gpu, egt_lib):
    _homogeneous(CD.make_ffn(W, matmul, bf16, act, "plain"), CD.ffn_gpu, gpu)


@pytest.mark.parametrize("cid", ["n9_de16", "n19_de32_relu", "n21_de64_sn64"])
def test_xtalk_backward_is_homogeneous(cid, gpu, egt_lib):
    """egt_xtalk_bwd behind xtalk_ffn at De 16, 32 and 64 (the last with s_n = 64: the backward's second walk); both upstream
    gradients scaled"""
    _homogeneous(CD.make_xtalk(cid, "plain"), CD.xtalk_gpu, gpu)


def test_head_backwards_are_homogeneous(gpu, egt_lib):
    _homogeneous(CD.make_edge_head(*CD.EDGE_HEAD_CASES[1], "plain"), CD.edge_head_gpu, gpu)
    _homogeneous(CD.make_node_head(*CD.NODE_HEAD_CASES[0], "plain"), CD.node_head_gpu, gpu)


@pytest.mark.parametrize("edge_dtype", ["fp32", "bf16"])
def test_edge_embedding_backward_is_homogeneous(edge_dtype, gpu, egt_lib):
    """egt_edge_embed_bwd (ZINC form: feature table + hop kernel + bias)"""
    from egt_amd import edge_embed
    B, N, De, K, V = 2, 21, 8, 4, 5
    g = CD.gen("edge_embed")
    adj = (torch.rand(B, N, N, generator=g) > 0.8).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float()
    fm = torch.where(adj > 0, torch.randint(0, V - 1, (B, N, N), generator=g), torch.tensor(-1))
    ps = [torch.randn(V, De, generator=g), torch.randn(K, De, generator=g) * 0.3, torch.randn(De, generator=g) * 0.2]
    de = torch.randn(B, N, N, De, generator=g)
    kw = {} if edge_dtype == "fp32" else dict(edge_dtype="bf16")

    def run(f):
        pg = [x.to(gpu).requires_grad_() for x in ps]
        e = edge_embed(fm.to(gpu), adj.to(gpu), *pg, **kw)
        e.backward((de * f).to(gpu).to(e.dtype))
        return [p.grad for p in pg]

    base = run(1.0)
    for k in (10, -10):
        for a, b in zip(run(2.0 ** k), base):
            assert float(b.abs().max()) > 0 and torch.equal(a, b * 2.0 ** k)
