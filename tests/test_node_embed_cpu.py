"""CPU checks of the node-input embedding (egt_node_embed_*, egt_amd/node_embed.py): the C-ABI boundary, argument validation
without a GPU, the composed ops against the fp64 oracle, and the admission of the GPU case table (tests/node_embed_cases.py):
a case is fair when the composed ops in fp32 on the CPU stay within 0.25 of util.FWD / util.BWD against the fp64 oracle (the
rule of tests/test_conditioning_cpu.py), so a kernel that fails is at least four times worse than plain fp32 arithmetic."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import node_embed_cases as NC
import test_capi
import util

ENTRY = ("egt_node_embed_supported", "egt_node_embed_workspace_bytes", "egt_node_embed_fwd", "egt_node_embed_bwd")
CAP = 0.25


def test_header_declares_and_library_exports_the_entry_points(egt_lib):
    from egt_amd import _lib as L
    syms = test_capi.declared_symbols()
    raw = C.CDLL(egt_lib._name)
    for s in ENTRY:
        assert s in syms and hasattr(raw, s) and s in L._PROTOS
    assert set(syms) == set(L._PROTOS)
    assert egt_lib.egt_abi_version() == 4


def test_struct_layouts_match_the_ctypes_mirrors(tmp_path):
    from egt_amd import _lib as L
    pairs = [("egt_node_embed_desc", L.NodeEmbedDesc), ("egt_node_embed_params", L.NodeEmbedParams)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "egt_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("consts %d %d %d %d %d %d %d\\n", EGT_NE_INT, EGT_NE_FLOAT, EGT_NE_PE_NONE, EGT_NE_PE_SVD, EGT_NE_PE_EIG, '
              'EGT_NE_TRANSFORM, EGT_NE_SIGNS);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(test_capi.REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.split(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert [int(x) for x in got["consts"].split()] == [L.NE_INT, L.NE_FLOAT, L.NE_PE_NONE, L.NE_PE_SVD, L.NE_PE_EIG, L.NE_TRANSFORM,
                                                       L.NE_SIGNS]


def _desc(**kw):
    from egt_amd.node_embed import node_embed_desc
    base = dict(B=2, N=9, Dh=64, nv=0, R=29, F_=0, pe_kind=None, T=0, sel=0, transform=False)
    base.update(kw)
    return node_embed_desc(**base)


SUPPORTED = [dict(Dh=w) for w in (16, 32, 48, 64)] + [
    dict(R=1), dict(R=32), dict(R=0, F_=1), dict(R=0, F_=8), dict(nv=16), dict(B=1, N=1), dict(B=128, N=188),
    dict(pe_kind="svd", T=16, sel=8, transform=True), dict(pe_kind="svd", T=32, sel=32, transform=True),
    dict(pe_kind="svd", T=32, sel=32, transform=False), dict(Dh=16, pe_kind="svd", T=8, sel=8, transform=False),
    dict(pe_kind="eig", T=20, sel=2), dict(pe_kind="eig", T=32, sel=32, transform=True), dict(Dh=16, pe_kind="eig", T=20, sel=16),
    dict(pe_kind="eig", T=20, sel=20, signs=True), dict(pe_kind="eig", T=20, sel=20, signs=True, sign_stride=64),
    dict(R=0, F_=5, nv=1, pe_kind="svd", T=16, sel=8, transform=True, signs=True),
]
UNSUPPORTED = [
    dict(Dh=80), dict(Dh=24), dict(Dh=0), dict(R=33), dict(R=0), dict(R=0, F_=9), dict(R=4, F_=2), dict(nv=17), dict(nv=-1),
    dict(B=0), dict(N=0), dict(Dh=16, pe_kind="svd", T=16, sel=9, transform=False),        # 2 sel > Dh without a Dense
    dict(Dh=16, pe_kind="eig", T=20, sel=17), dict(pe_kind="svd", T=40, sel=33, transform=True), dict(pe_kind="eig", T=7, sel=8),
    dict(pe_kind="eig", T=20, sel=0), dict(pe_kind="bogus", T=20, sel=2), dict(transform=True), dict(T=3),
    dict(pe_kind="eig", T=20, sel=8, signs=True, sign_stride=7), dict(B=1 << 20, N=1 << 6),
]


@pytest.mark.parametrize("kw", SUPPORTED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_supported_geometries(egt_lib, kw):
    d = _desc(**kw)
    assert egt_lib.egt_node_embed_supported(C.byref(d)) == 1
    ws = egt_lib.egt_node_embed_workspace_bytes(C.byref(d))
    assert ws > 0 and ws % 4 == 0
    assert ws <= 4 * 256 * (2 * 32 + 8 + 1 + 32) * 64          # at most 256 partials of at most 105 rows of Dh floats


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_unsupported_geometries(egt_lib, kw):
    from egt_amd import _lib as L
    d = _desc(**kw)
    assert egt_lib.egt_node_embed_supported(C.byref(d)) == 0
    assert egt_lib.egt_node_embed_workspace_bytes(C.byref(d)) == 0
    p = L.NodeEmbedParams()
    assert egt_lib.egt_node_embed_fwd(C.byref(d), C.byref(p), *([None] * 6)) in (L.EGT_E_SHAPE, L.EGT_E_FLAGS)
    assert b"node embed" in egt_lib.egt_last_error_string()
    assert egt_lib.egt_node_embed_bwd(C.byref(d), None, None, None, None, C.byref(p), None, None) in (L.EGT_E_SHAPE, L.EGT_E_FLAGS)


def test_null_arguments_and_flag_bits(egt_lib):
    from egt_amd import _lib as L
    assert egt_lib.egt_node_embed_supported(None) == 0 and egt_lib.egt_node_embed_workspace_bytes(None) == 0
    d = _desc(pe_kind="svd", T=16, sel=8, transform=True, signs=True, nv=1)
    p = L.NodeEmbedParams()
    one = C.c_void_p(64)                                           # a non-NULL address: validation never dereferences
    assert egt_lib.egt_node_embed_fwd(None, C.byref(p), *([one] * 5), None) == L.EGT_E_NULL
    assert egt_lib.egt_node_embed_fwd(C.byref(d), None, *([one] * 5), None) == L.EGT_E_NULL
    assert egt_lib.egt_node_embed_fwd(C.byref(d), C.byref(p), *([one] * 5), None) == L.EGT_E_NULL      # node_emb NULL
    assert b"node_emb of params" in egt_lib.egt_last_error_string()
    for f in L.NODE_EMBED_PARAM_FIELDS:
        setattr(p, f, 64)
    p.node_emb_bias = None                                          # integer kind: never used
    for missing in range(5):                                        # features, pe, signs, h_out, mask_out
        a = [one] * 5
        a[missing] = None
        assert egt_lib.egt_node_embed_fwd(C.byref(d), C.byref(p), *a, None) == L.EGT_E_NULL, missing
    p.virtual_node_emb = None
    assert egt_lib.egt_node_embed_fwd(C.byref(d), C.byref(p), *([one] * 5), None) == L.EGT_E_NULL
    assert b"virtual_node_emb" in egt_lib.egt_last_error_string()
    p.virtual_node_emb = 64
    for missing in range(6):                                        # features, pe, signs, d_h, (grads), workspace
        a = [one, one, one, one, C.byref(p), one]
        a[missing] = None
        assert egt_lib.egt_node_embed_bwd(C.byref(d), *a, None) == L.EGT_E_NULL, missing
    d.flags |= 0x10
    assert egt_lib.egt_node_embed_supported(C.byref(d)) == 0
    assert egt_lib.egt_node_embed_fwd(C.byref(d), C.byref(p), *([one] * 5), None) == L.EGT_E_FLAGS
    d = _desc()
    d.reserved = 1
    assert egt_lib.egt_node_embed_supported(C.byref(d)) == 0


def test_python_queries_agree_with_the_library(egt_lib):
    from egt_amd.node_embed import node_embed_supported
    assert node_embed_supported(128, 64, 64, 1, 29, 0, "svd", 16, 8, True)
    assert node_embed_supported(128, 150, 64, 1, 0, 5, "svd", 16, 8, True)
    assert node_embed_supported(128, 188, 64, 0, 4, 0, "eig", 20, 2, False)
    assert not node_embed_supported(128, 64, 80, 1, 29)
    for name, c in NC.CASES.items():
        kind, sel, T, tr = c.get("pe") or (None, 0, 0, False)
        assert node_embed_supported(c["B"], c["N"], c["Dh"], c["nv"], c.get("R", 0), c.get("F", 0), kind, T, sel, tr), name


@pytest.fixture(scope="module")
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("signs", [True, False], ids=["signs", "nosigns"])
@pytest.mark.parametrize("name", list(NC.CASES))
def test_composed_equals_the_oracle_and_the_case_is_fair(name, signs, _one_thread):
    from egt_amd.node_embed import node_embed_composed
    c = NC.make(name)
    h_ref, mask_ref, g_ref, gpos_ref = NC.oracle(c, signs)
    # fp64: the composed ops ARE the oracle's statements
    a, p = NC.args(c, torch.float64, signs=signs)
    h, mask = node_embed_composed(*a)
    assert h.shape == (c["B"], c["nv"] + c["N"], c["Dh"]) and mask.dtype == torch.bool and torch.equal(mask, mask_ref)
    util.assert_close(h, h_ref, rtol=1e-12, arel=1e-12, name=f"{name}: h (fp64)")
    for up, ref in (("d_h", g_ref), ("d_h_pos", gpos_ref)):
        got = NC.grads(h, p, c[up].double())
        assert set(got) == set(ref)
        for k in ref:
            util.assert_close(got[k], ref[k], rtol=1e-12, arel=1e-12, name=f"{name}: d {k} (fp64, {up})", zero_atol=1e-12)
    # fp32: the admission rule of the GPU table
    a, p = NC.args(c, torch.float32, signs=signs)
    h, mask = node_embed_composed(*a)
    assert torch.equal(mask, mask_ref)
    worst = {"h": util.margin(h, h_ref, rtol=util.FWD["rtol"], arel=util.FWD["arel"])}
    for up, ref in (("d_h", g_ref), ("d_h_pos", gpos_ref)):
        got = NC.grads(h, p, c[up])
        for k in ref:
            worst[f"{k}/{up}"] = util.margin(got[k], ref[k], rtol=util.BWD["rtol"], arel=util.BWD["arel"])
    bad = {k: v for k, v in worst.items() if not v <= CAP}
    assert not bad, f"{name}: plain fp32 already uses {bad} of the tolerance (cap {CAP})"


def test_table_reaches_what_it_is_meant_to():
    """the properties the shapes were chosen for"""
    c = NC.make("empty_n65_vn1_svd")
    assert c["counts"] == [65, 0, 17] and c["N"] > 64 and c["pe_t"].shape[2] > c["pe"][1]
    assert (c["features"][1] == -1).all()
    assert NC.make("w32_nv16")["nv"] > NC.make("w32_nv16")["N"]
    b = NC.make("b37_n40_svd_vn1")
    assert b["B"] * b["N"] > 128 * 8                                   # several backward workgroups
    assert all((NC.make(n)["d_h_pos"] > 0).all() for n in NC.CASES)
    for n in NC.CASES:
        c = NC.make(n)
        if "R" in NC.CASES[n] and c["N"] > 1 and n != "w32_nv16":
            assert (c["features"] == -1).any(), n                      # padded rows: they add to table row 0 / the biases


MODELS = [("zinc", dict(use_svd=True, num_svd_features=16, sel_svd_features=8, transform_svd=True, random_neg=True, num_virtual_nodes=1)),
          ("zinc", dict(use_eig=True, num_eig_features=20, sel_eig_features=8, random_neg=True)),
          ("pattern", dict(use_eig=True, num_eig_features=20, sel_eig_features=2)), ("cluster", {}),
          ("cifar10", dict(use_svd=True, num_svd_features=16, sel_svd_features=8, transform_svd=True, num_virtual_nodes=1)),
          ("mnist", {})]


@pytest.mark.parametrize("which,kw", MODELS, ids=[f"{m}-{'svd' if k.get('use_svd') else 'eig' if k.get('use_eig') else 'plain'}"
                                                  for m, k in MODELS])
def test_models_build_and_their_node_path_runs_on_the_cpu(which, kw):
    """every model class still builds; `embeddings` has no CPU path (the mask producers are kernels), the rest of the node path
    -- positional, with_virtual_nodes -- equals node_embed_composed on the model's own parameters"""
    from egt_amd import model as M
    from egt_amd.node_embed import node_embed_composed
    cls = dict(zinc=M.ZincDCTransformer, pattern=M.PatternDCTransformer, cluster=M.ClusterDCTransformer,
               cifar10=M.Cifar10DCTransformer, mnist=M.MnistDCTransformer)[which]
    torch.manual_seed(0)
    m = cls(model_width=64, edge_width=8, model_height=2, **kw)
    B, N = 2, 7
    g = torch.Generator().manual_seed(1)
    is_float = which in ("cifar10", "mnist")
    feat = torch.randn(B, N, m.node_emb.kernel.shape[0], generator=g) if is_float else \
        torch.randint(0, m.node_emb.shape[0] - 1, (B, N), generator=g, dtype=torch.int32)
    feat[1, 5:] = -1
    sv = torch.randn(B, N, 16, 2, generator=g) if kw.get("use_svd") else None
    ev = torch.randn(B, N, 20, generator=g) if kw.get("use_eig") else None
    kind = "svd" if sv is not None else ("eig" if ev is not None else None)
    emb, bias = m._node_params()
    if is_float:
        real = (feat != m.mask_value).any(-1)
        h0 = m.node_emb(feat * real[..., None].to(feat.dtype))
    else:
        h0 = torch.nn.functional.embedding((feat + 1).long(), m.node_emb)
    m.train()
    torch.manual_seed(5)
    got = m.with_virtual_nodes(m.positional(h0, sv, ev))
    torch.manual_seed(5)                                             # the same sign stream
    sel = m.cfg[f"sel_{kind}_features"] if kind else 0
    signs = None
    if kind and m.cfg["random_neg"]:
        w = sel if m.cfg[f"transform_{kind}"] else max(sel, 32 if kind == "svd" else 64)
        signs = torch.where(torch.rand(B, 1, w, 1, device=feat.device) < 0.5, -1.0, 1.0)
        signs = signs if kind == "svd" else signs[..., 0]
    want, mask = node_embed_composed(feat, emb, bias, sv if kind == "svd" else ev, kind, sel, m._pe_dense(), signs,
                                     m.virtual_node_emb if m.num_virtual_nodes else None, getattr(m, "mask_value", -1.0))
    assert torch.equal(got, want)
    assert mask.shape == (B, m.num_virtual_nodes + N) and not mask[1, m.num_virtual_nodes + 5:].any() and mask[0].all()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.node_input(feat, sv, ev)


def test_switch_is_read_once(monkeypatch):
    from egt_amd import node_embed as NE
    monkeypatch.setattr(NE, "_NO_NODE_EMBED", None)
    monkeypatch.setenv("EGT_NO_NODE_EMBED", "1")
    assert NE.node_embed_disabled()
    monkeypatch.setenv("EGT_NO_NODE_EMBED", "0")
    assert NE.node_embed_disabled()                                  # read once per process
    monkeypatch.setattr(NE, "_NO_NODE_EMBED", None)
    assert not NE.node_embed_disabled()
    monkeypatch.setattr(NE, "_NO_NODE_EMBED", None)


# ------------------------------------------------------------- the reference pin of the positional-encoding path -----
import node_embed_reference as NRF  # noqa: E402
from oracle import ref_exec as RX  # noqa: E402

REL = 1e-12          # the rule of tests/test_reference_exec_cpu.py: |a - r| <= 1e-12 max|r| per tensor, both sides fp64


def _within(name, a, r):
    a, r = a.double(), r.double()
    assert a.shape == r.shape, name
    mx = float(r.abs().max())
    bound = REL * (mx if mx >= 1e-9 else 1.0)       # identically zero in exact arithmetic: the bound at magnitude 1
    err = float((a - r).abs().max())
    assert err <= bound, f"{name}: |oracle - reference| up to {err:.3e} > {bound:.3e} (max|reference| {mx:.3e})"


@pytest.mark.parametrize("name", list(NRF.CASES))
def test_oracle_matches_the_reference_with_positional_encodings(name):
    """oracle/egt_model_oracle.py (svd_embedding / eig_embedding inside zinc_forward) against what the reference's
    DCSVDTransformer(use_svd=True) / DCEigTransformer(use_eig=True) computed: output, loss, every parameter gradient"""
    fix = NRF.load(name)
    inp, params, _ = NRF.model_inputs(name)
    for k, v in inp.items():
        assert torch.equal(v, fix["inputs"][k].to(v.dtype)), f"inputs/{k}: the recipe no longer gives the fixture's array"
    assert set(params) == set(fix["weights"])
    for k, v in params.items():
        assert torch.equal(v, fix["weights"][k]), f"weights/{k}: the recipe no longer gives the fixture's array"
    kind = NRF.CASES[name]["kind"]
    assert (f"{kind}_emb.kernel" in params) == (kind == "svd")
    got, _ = NRF.oracle(fix, name)
    assert set(got) == set(fix["out"])
    for k, r in fix["out"].items():
        assert r.dtype == torch.float64
        _within(f"{name}: {k}", got[k], r)
    if kind == "svd":                                # the encoding reaches the output: its Dense is trained
        assert float(fix["out"]["d/svd_emb.kernel"].abs().max()) > 0
    for f in os.listdir(NRF.DIR):
        assert os.path.getsize(os.path.join(NRF.DIR, f)) < (1 << 20)


@pytest.mark.skipif(not RX.available(), reason="no reference tree (EGT_REFERENCE_DIR)")
def test_regenerated_fixture_equals_the_committed_one(tmp_path):
    """the generator, run again in a child process (it registers stand-in modules), writes the committed numbers"""
    import numpy as np
    gen = os.path.join(test_capi.REPO, "tests", "golden", "make_node_embed_golden.py")
    code = f"import runpy, sys; sys.argv = ['x']; import node_embed_reference as N; N.DIR = {str(tmp_path)!r}; runpy.run_path({gen!r}, run_name='__main__')"
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(test_capi.REPO, "tests"), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in NRF.CASES:
        new, old = np.load(tmp_path / f"{name}.npz"), np.load(os.path.join(NRF.DIR, f"{name}.npz"))
        assert set(new.files) == set(old.files)
        for k in old.files:
            if k.startswith("out/"):
                _within(f"{name}: {k}", torch.from_numpy(new[k]), torch.from_numpy(old[k]))
            else:
                assert np.array_equal(new[k], old[k]), k
