"""The large-head block operator (egt_pair_block_*) without a GPU: header / prototypes / exports, coverage and size queries,
argument errors, the launch plan as text against its host restatement, the route switch, and the fairness of the table's inputs."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import pair_block_cases as PB
from util import FWD, BWD, margin

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"egt_pair_block_supported": 1, "egt_pair_block_launch_form": 1, "egt_pair_block_saved_bytes": 1,
           "egt_pair_block_workspace_bytes": 1, "egt_pair_block_fwd": 10, "egt_pair_block_bwd": 13}


def _base(L):
    """the descriptor of tests/test_capi.py::test_pair_entry_points_validate_without_gpu"""
    return L.BlockDesc(B=8, N=512, H=8, d=64, De=32, dtype=L.EGT_F32, flags=L.BF_GATE | L.BF_CLIP, clip_lo=-5, clip_hi=5,
                       random_mask_prob=0.0, ln_eps=1e-3, reserved=0, seed=0, seed_device=None)


def _refusals(L):
    """the refusals of tests/test_pair_gpu.py::test_pair_no_clip_and_refusals, and the device seed"""
    return (("d", 32), ("De", 64), ("H", 4), ("flags", L.BF_CLIP), ("flags", L.BF_GATE | L.BF_ATTN_MASK), ("dtype", L.EGT_BF16),
            ("flags", L.BF_GATE | L.BF_CLIP | L.BF_SEED_DEVICE))


def test_header_protos_and_exports(egt_lib):
    from egt_amd import _lib as L
    header = open(os.path.join(REPO, "include", "egt_amd.h")).read()
    assert re.search(r"#define EGT_ABI_VERSION 4\b", header) and egt_lib.egt_abi_version() == 4
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\b" + name + r"\(([^;]*?)\);", header, re.S)
        assert m, f"{name} is not declared in include/egt_amd.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in L._PROTOS and len(L._PROTOS[name][1]) == nargs, name
        assert getattr(egt_lib, name) is not None
    # egt_block_fwd / egt_block_bwd's signature without attn_mask / rand_mask
    assert len(L._PROTOS["egt_pair_block_fwd"][1]) == len(L._PROTOS["egt_block_fwd"][1]) - 2
    assert len(L._PROTOS["egt_pair_block_bwd"][1]) == len(L._PROTOS["egt_block_bwd"][1]) - 2
    assert "egt_pair_node.hip" in __import__("egt_amd.build", fromlist=["SOURCES"]).SOURCES


def test_supported_equals_the_pair_operator(egt_lib):
    from egt_amd import _lib as L
    d = _base(L)
    assert egt_lib.egt_pair_supported(C.byref(d)) == 1 and egt_lib.egt_pair_block_supported(C.byref(d)) == 1
    assert egt_lib.egt_pair_block_saved_bytes(C.byref(d)) > 0 and egt_lib.egt_pair_block_workspace_bytes(C.byref(d)) > 0
    # saved embeds the pair operator's shared workspace whole, next to QKV, V_att, the attention and LayerNorm row statistics
    sh = L.BlockDesc.from_buffer_copy(d); sh.reserved = L.ATTN_WS_SHARED
    R = 8 * 512
    assert egt_lib.egt_pair_block_saved_bytes(C.byref(d)) == 4 * R * (1536 + 512 + 32 + 2) + egt_lib.egt_pair_workspace_bytes(C.byref(sh))
    for field, val in _refusals(L):
        d2 = L.BlockDesc.from_buffer_copy(d)
        setattr(d2, field, val)
        assert egt_lib.egt_pair_block_supported(C.byref(d2)) == egt_lib.egt_pair_supported(C.byref(d2)) == 0, (field, val)
        assert egt_lib.egt_pair_block_saved_bytes(C.byref(d2)) == 0 and egt_lib.egt_pair_block_workspace_bytes(C.byref(d2)) == 0
        assert egt_lib.egt_pair_block_launch_form(C.byref(d2)) is None
    for B, N, _ in PB.TABLE:
        t = PB.desc(B, N)
        assert egt_lib.egt_pair_block_supported(C.byref(t)) == egt_lib.egt_pair_supported(C.byref(t)) == 1


def test_argument_errors(egt_lib):
    from egt_amd import _lib as L
    d = _base(L)
    prm = L.BlockParams()
    assert egt_lib.egt_pair_block_fwd(C.byref(d), C.byref(prm), *([None] * 8)) == L.EGT_E_NULL
    assert b"NULL" in egt_lib.egt_last_error_string()
    assert egt_lib.egt_pair_block_bwd(C.byref(d), C.byref(prm), *([None] * 8), C.byref(prm), None, None) == L.EGT_E_NULL
    assert egt_lib.egt_pair_block_fwd(C.byref(d), None, *([None] * 8)) == L.EGT_E_NULL
    # every buffer present, a parameter pointer missing (host memory is fine: the check precedes any launch)
    buf = (C.c_char * 64)()
    one = C.cast(buf, C.c_void_p)
    assert egt_lib.egt_pair_block_fwd(C.byref(d), C.byref(prm), one, one, one, one, one, one, one, None) == L.EGT_E_NULL
    assert b"parameter pointer" in egt_lib.egt_last_error_string()
    r = L.BlockDesc.from_buffer_copy(d); r.reserved = L.ATTN_WS_SHARED          # the block shares the pair workspace itself
    assert egt_lib.egt_pair_block_fwd(C.byref(r), C.byref(prm), *([None] * 8)) == L.EGT_E_FLAGS
    d.d = 8                                                                      # the d <= 8 geometry belongs to egt_block_*
    assert egt_lib.egt_pair_block_supported(C.byref(d)) == 0
    assert egt_lib.egt_pair_block_fwd(C.byref(d), C.byref(prm), *([None] * 8)) == L.EGT_E_SHAPE
    assert b"large-head block" in egt_lib.egt_last_error_string()
    assert egt_lib.egt_pair_block_bwd(C.byref(d), C.byref(prm), *([None] * 8), C.byref(prm), None, None) == L.EGT_E_SHAPE
    assert egt_lib.egt_pair_block_fwd(None, C.byref(prm), *([None] * 8)) == L.EGT_E_SHAPE


def test_launch_form_is_the_host_plan(egt_lib):
    """parses; equals the restatement of the plan for R = 1 .. 20000; a function of R only"""
    for R in range(1, 20001):
        B, N = (R, 1) if R % 7 else (R // 7, 7)
        text = egt_lib.egt_pair_block_launch_form(C.byref(PB.desc(B, N)))
        assert text is not None and text.decode() == PB.form(R), (R, text)
    p = PB.parse(PB.form(1080))
    assert p == dict(tile=128, tiles=9, tile_ragged=True, rpc=256, chunks=5, chunk_ragged=True, ln_rows=64, ln_parts=17, reduce=1)
    for R, shapes in ((1024, ((64, 16), (32, 32), (2, 512), (1024, 1))), (1080, ((40, 27), (27, 40), (10, 108)))):
        forms = set()
        for B, N in shapes:
            for flags_extra in (0, 0x4):                                          # EGT_BF_TRAINING
                from egt_amd import _lib as L
                d = PB.desc(B, N, flags=L.BF_GATE | L.BF_CLIP | flags_extra)
                forms.add(egt_lib.egt_pair_block_launch_form(C.byref(d)))
        assert forms == {PB.form(R).encode()}, forms
    for R in range(1, 20001):            # the plan's own invariants: every row in exactly one chunk, chunk starts on the k step
        p = PB.plan(R)
        assert p["rpc"] % PB.K_STEP == 0 and 1 <= p["chunks"] <= PB.MAX_CHUNKS and (p["chunks"] - 1) * p["rpc"] < R <= p["chunks"] * p["rpc"]


def test_table_reaches_every_class(egt_lib):
    seen = set()
    for B, N, nodes in PB.TABLE:
        assert len(nodes) == B and all(0 <= n <= N for n in nodes)
        text = egt_lib.egt_pair_block_launch_form(C.byref(PB.desc(B, N))).decode()
        p = PB.parse(text)
        assert {k: p[k] for k in ("tiles", "tile_ragged", "rpc", "chunks", "chunk_ragged", "ln_parts", "reduce")} == PB.plan(B * N)
        seen |= PB.classes(p)
    assert seen == PB.ALL_CLASSES, PB.ALL_CLASSES - seen
    assert any(0 in nodes for _, _, nodes in PB.TABLE), "a graph with no node"


def test_node_route_honours_the_switch(egt_lib):
    code = ("from egt_amd import EGTBlock\nfrom egt_amd.pair import node_route\n"
            "big = EGTBlock(model_width=512, edge_width=32, num_heads=8)\nsmall = EGTBlock(model_width=64, edge_width=32, num_heads=8)\n"
            "print(node_route(big, 2, 16), node_route(small, 2, 16), node_route(big, 2, 16))")
    out = {}
    for val in (None, "0", "1"):
        env = {k: v for k, v in os.environ.items() if k != "EGT_PAIR_NODE"}
        if val is not None:
            env["EGT_PAIR_NODE"] = val
        r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[val] = r.stdout.split()
    assert out[None] == ["torch", "torch", "torch"] and out["0"] == ["torch", "torch", "torch"]
    assert out["1"] == ["library", "torch", "library"]          # only where egt_pair_block_supported covers the block


@pytest.mark.parametrize("i", range(len(PB.TABLE)), ids=PB.IDS)
def test_fairness_of_the_table_rows(i):
    """the fp32 oracle stays within conditioning.CAP of util.FWD / util.BWD on every row: the tolerances are the kernels' to use"""
    from conditioning import CAP
    r64, r32 = PB.oracle(i), PB.oracle(i, torch.float32)
    worst = {}
    for k, tol in (("h_out", FWD), ("e_out", FWD), ("dh", BWD), ("de", BWD)):
        worst[k] = margin(r32[k], r64[k], rtol=tol["rtol"], arel=tol["arel"])
    for k in r64["dparams"]:
        if float(r64["dparams"][k].abs().max()) >= 1e-9:
            worst[k] = margin(r32["dparams"][k], r64["dparams"][k], rtol=BWD["rtol"], arel=BWD["arel"])
    bad = {k: round(v, 3) for k, v in worst.items() if v > CAP}
    assert not bad, bad
