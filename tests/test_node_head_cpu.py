"""Node-classification head without a GPU: the shared inputs meet their conditions, the composed head against the fp64
restatement (node_head_ref.py), the library's coverage answers and refusals, the struct layouts, and the models'
classification_loss on CPU tensors (the composed path) against forward + weighted_sparse_xent_loss + the metric sums."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import node_head_ref as NR
from util import assert_close, FWD, BWD

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(64, 64, 6, "elu", True), (64, 64, 2, "elu", True), (48, 48, 6, "relu", True), (16, 64, 3, "elu", False)]   # W, width -> hidden, C, act, LN


def test_shared_inputs_meet_their_conditions():
    for W, width, Cn, act, ln in CASES:
        x = NR.make_inputs(3, 19, W, Cn)
        mask, target = x["mask"], x["target"]
        full, part, none, last = NR.tile_census(mask)
        assert full >= 1 and part >= 1 and last == 57 - 48 == 9, (full, part, none, last)    # 57 rows: 3 full-size tiles + a ragged one
        assert bool(mask[-1].any()) and bool(mask.reshape(-1)[48:].any()), "the ragged last tile holds real rows"
        assert int(mask[1].sum()) == 0, "one graph is masked entirely"
        assert sorted(target[mask].unique().tolist()) == list(range(Cn)), "every class occurs among the unmasked targets"
        junk = target[~mask]
        assert int((junk == -1).sum()) > 0 and int((junk >= Cn).sum()) > 0
        p64 = tuple(None if p is None else p.double() for p in NR.head_params(W, width, Cn, ln))
        _, z = NR.ref_stats(x["h"].double(), target, mask, x["class_weights"].double(), p64, act)
        assert NR.top2_gap(z, mask) > 1e-3, "the hit count is unambiguous"
    big = NR.make_inputs(4, 70, 64, 6)
    assert NR.tile_census(big["mask"])[2] >= 3, "tiles without a real row (skipped before h is loaded)"
    assert NR.workgroups(4, 70) == (4, 5) and NR.workgroups(3, 19) == (1, 4) and NR.workgroups(128, 188) == (376, 4)
    assert NR.tile_census(NR.make_inputs(2, 16, 64, 6)["mask"]) == (2, 0, 0, 16)


@pytest.mark.parametrize("W,width,Cn,act,ln", CASES)
def test_composed_head_equals_the_fp64_restatement(W, width, Cn, act, ln):
    from egt_amd.node_head import node_head_composed
    x = NR.make_inputs(3, 19, W, Cn)
    params = NR.head_params(W, width, Cn, ln)
    h64 = x["h"].double().requires_grad_()
    p64 = tuple(None if p is None else p.double().requires_grad_() for p in params)
    st64, _ = NR.ref_stats(h64, x["target"], x["mask"], x["class_weights"].double(), p64, act)
    gr = torch.autograd.grad(st64[0], [h64] + [p for p in p64 if p is not None])
    h = x["h"].clone().requires_grad_()
    ps = tuple(None if p is None else p.clone().requires_grad_() for p in params)
    st = node_head_composed(h, x["target"], x["mask"], x["class_weights"], ps, act)
    assert st.shape == (3,) and st.dtype == torch.float32
    gc = torch.autograd.grad(st[0], [h] + [p for p in ps if p is not None])
    st, st64 = st.detach(), st64.detach()
    assert_close(st[0], st64[0], name="loss sum", **FWD)
    assert float(st[1]) == float(st64[1]) and float(st[2]) == float(st64[2]) == float(x["mask"].sum())
    names = ("d_h",) + (NR.NAMES if ln else NR.NAMES[2:])
    for n, a, r in zip(names, gc, gr):
        assert_close(a, r, name=n, **BWD)
    assert float(gc[0][~x["mask"]].abs().max()) == 0.0
    # the composed head in fp64 IS the restatement
    st_d = node_head_composed(h64, x["target"], x["mask"], x["class_weights"].double(), p64, act)
    assert_close(st_d, st64, name="fp64 composed", rtol=1e-12, arel=1e-12)


def test_library_coverage(egt_lib):
    from egt_amd import _lib as L
    from egt_amd.node_head import node_head_desc, node_head_supported
    for W in (16, 32, 48, 64):
        for m0, m1 in ((24, 12), (32, 16)):
            for Cn in (2, 3, 6, 16):
                for act in ("elu", "relu"):
                    for ln in (True, False):
                        d = node_head_desc(3, 19, W, m0, m1, Cn, act, ln)
                        assert egt_lib.egt_node_head_supported(C.byref(d)) == 1, (W, m0, m1, Cn, act, ln)
                        assert egt_lib.egt_node_head_workspace_bytes(C.byref(d)) > 0
    assert node_head_supported(128, 188, 64, 32, 16, 6)
    for bad in (dict(W=80, M0=40, M1=20), dict(W=80), dict(M0=16, M1=8), dict(C_=1), dict(C_=17), dict(activation="lrelu"), dict(W=8)):
        kw = dict(B=3, N=19, W=64, M0=32, M1=16, C_=6, activation="elu", layernorm=True)
        kw.update(bad)
        d = node_head_desc(**kw)
        assert egt_lib.egt_node_head_supported(C.byref(d)) == 0, bad
        assert egt_lib.egt_node_head_workspace_bytes(C.byref(d)) == 0, bad
    d = node_head_desc(1 << 16, 1 << 15, 64, 32, 16, 6)                       # B N = 2^31
    assert egt_lib.egt_node_head_supported(C.byref(d)) == 0
    d = node_head_desc((1 << 16) - 1, 1 << 15, 64, 32, 16, 6)                 # just inside
    assert egt_lib.egt_node_head_supported(C.byref(d)) == 1
    # the workspace follows the chunking rule: image + 3 G + (G + 1) PG floats
    G, _ = NR.workgroups(4, 70)
    img, pg = 64 * 36 + 32 * 20 + 16 * 20 + 64, 64 * 32 + 32 * 16 + 16 * 16 + 64
    d = node_head_desc(4, 70, 64, 32, 16, 6)
    assert egt_lib.egt_node_head_workspace_bytes(C.byref(d)) == 4 * (img + 3 * G + (G + 1) * pg)
    assert L.ABI_VERSION == 4 and egt_lib.egt_abi_version() == 4


def test_refusals_without_a_gpu(egt_lib):
    """argument checks run before any launch: error codes as the other entry points give them"""
    from egt_amd import _lib as L
    from egt_amd.node_head import node_head_desc
    ok = node_head_desc(3, 19, 64, 32, 16, 6)
    one = C.c_void_p(16)                                                       # any non-NULL value: never dereferenced here
    prm = L.NodeHeadParams(*([16] * 8))
    noln = L.NodeHeadParams(None, None, *([16] * 6))

    def fwd(d, p=prm, h=one, target=one, mask=one, cw=one, stats=one, ws=one):
        return egt_lib.egt_node_head_fwd(C.byref(d) if d is not None else None, C.byref(p) if p is not None else None, h, target,
                                         mask, cw, stats, ws, None)

    def bwd(d, p=prm, g=prm, d_loss=one, d_h=one):
        return egt_lib.egt_node_head_bwd(C.byref(d), C.byref(p), one, one, one, one, d_loss, d_h,
                                         C.byref(g) if g is not None else None, one, None)

    assert fwd(None) == L.EGT_E_NULL
    assert fwd(ok, p=None) == L.EGT_E_NULL
    for k in ("h", "target", "mask", "cw", "stats", "ws"):
        assert fwd(ok, **{k: None}) == L.EGT_E_NULL, k
    assert b"class_weights" in egt_lib.egt_last_error_string()
    assert fwd(ok, p=noln) == L.EGT_E_NULL and b"gamma/beta" in egt_lib.egt_last_error_string()
    assert bwd(ok, d_loss=None) == L.EGT_E_NULL and bwd(ok, d_h=None) == L.EGT_E_NULL and bwd(ok, g=None) == L.EGT_E_NULL
    assert bwd(ok, g=noln) == L.EGT_E_NULL
    d = node_head_desc(3, 19, 64, 32, 16, 6); d.flags = 0x5
    assert fwd(d) == L.EGT_E_FLAGS and bwd(d) == L.EGT_E_FLAGS and egt_lib.egt_node_head_supported(C.byref(d)) == 0
    d = node_head_desc(3, 19, 64, 32, 16, 6); d.reserved = 1
    assert fwd(d) == L.EGT_E_FLAGS
    d = node_head_desc(3, 19, 80, 32, 16, 6)
    assert fwd(d) == L.EGT_E_SHAPE and b"{16,32,48,64}" in egt_lib.egt_last_error_string()
    d = node_head_desc(3, 19, 64, 16, 8, 6)
    assert fwd(d) == L.EGT_E_SHAPE and b"(M0, M1)" in egt_lib.egt_last_error_string()
    assert fwd(node_head_desc(3, 19, 64, 32, 16, 17)) == L.EGT_E_SHAPE and bwd(node_head_desc(3, 19, 64, 32, 16, 1)) == L.EGT_E_SHAPE
    assert fwd(node_head_desc(0, 19, 64, 32, 16, 6)) == L.EGT_E_SHAPE
    with pytest.raises(AssertionError):
        L.check(L.EGT_E_SHAPE)


def test_struct_layouts_match_the_ctypes_mirrors(tmp_path):
    from egt_amd import _lib as L
    pairs = [("egt_node_head_desc", L.NodeHeadDesc), ("egt_node_head_params", L.NodeHeadParams)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "egt_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("flag %d\\n", EGT_NH_LAYERNORM);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert [f for f, _ in L.NodeHeadDesc._fields_] == ["B", "N", "W", "M0", "M1", "C", "activation", "flags", "ln_eps", "reserved"]
    assert int(got["flag"]) == L.NH_LAYERNORM


class _Pass(torch.nn.Module):
    """stands in for the layers of a model on the CPU (the attention blocks have no CPU path)"""

    def forward(self, h, e, mask, attn_mask, skip_last_edge_ffn=True):
        return h, e


def _cpu_model(cls, h, mask, **kw):
    """a model whose embeddings / layers are replaced by fixed tensors: forward and classification_loss share them"""
    model = cls(model_width=h.shape[-1], edge_width=8, model_height=1, upto_hop=2, random_mask_prob=0.0, **kw)
    e = torch.zeros(h.shape[0], h.shape[1], h.shape[1], 8)
    model.embeddings = lambda nf, fm, adj: (h, e, mask)
    model.layers = _Pass()
    return model


@pytest.mark.parametrize("which,width,Cn", [("cluster", 64, 6), ("pattern", 48, 2), ("pattern", 32, 2)])
def test_classification_loss_on_cpu_equals_forward_plus_loss(which, width, Cn, egt_lib):
    from egt_amd import ClusterDCTransformer, PatternDCTransformer, weighted_sparse_xent_loss
    x = NR.make_inputs(3, 19, width, Cn)
    torch.manual_seed(3)
    model = _cpu_model(ClusterDCTransformer if which == "cluster" else PatternDCTransformer, x["h"], x["mask"])
    assert model.target.kernel.shape[1] == Cn
    with torch.no_grad():
        for p in model.head_params():
            p.add_(0.1 * torch.randn_like(p))
    assert not model.node_head_fused(x["h"]), "CPU tensors take the composed head"
    nf = torch.where(x["mask"], torch.zeros_like(x["target"]), torch.full_like(x["target"], -1)).int()
    adj = torch.zeros(3, 19, 19)
    tgt = torch.where(x["mask"], x["target"], torch.zeros_like(x["target"]))          # (the old path reads every target)
    loss, stats, aux = model.classification_loss(nf, adj, x["target"], x["class_weights"])
    assert aux == {} and stats.shape == (3,)
    g_new = torch.autograd.grad(loss, [p for p in model.head_params()])
    # the batch_loss of before: forward + weighted_sparse_xent_loss + the metric sums
    logits, mask = model(nf, adj, return_mask=True)
    old = weighted_sparse_xent_loss(logits, tgt, mask, x["class_weights"])
    g_old = torch.autograd.grad(old, [p for p in model.head_params()])
    m = mask.to(logits.dtype)
    hit = ((logits.argmax(-1) == tgt).to(logits.dtype) * m).sum()
    logp = torch.log_softmax(logits.detach(), -1).gather(-1, tgt.clamp(min=0).long()[..., None])[..., 0]
    xs = (-(logp) * x["class_weights"][tgt.clamp(min=0).long()] * m).sum()
    tight = dict(rtol=1e-5, arel=1e-6)                                               # fp32 sums in another order
    assert_close(loss, old, name="loss", **tight)
    assert_close(stats[0], xs, name="xent sum", **tight)
    stats = stats.detach()
    assert float(stats[1]) == float(hit) and float(stats[2]) == float(m.sum())
    assert abs(float(loss.detach()) - float(stats[0]) / 57) <= 1e-7 * abs(float(loss.detach())), "SUM_OVER_BATCH_SIZE counts the padded slots"
    for a, b, n in zip(g_new, g_old, NR.NAMES):
        assert_close(a, b, name=n, **tight)
