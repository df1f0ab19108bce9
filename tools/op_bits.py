#!/usr/bin/env python3
"""A sha256 per output tensor of single ops, over the cases of their GPU tests, for comparing two builds of the library bit by bit.
One process loads one library: run it once per build (each run under its own time limit, chained with &&) and diff the listings.

    python tools/op_bits.py [--ops head,embed,block,ffn,attn,attn_bf16,pair] [--lib path/to/libegt_amd.so] > listing.txt      (--lib: the EGT_AMD_LIB of this process)
    python tools/op_bits.py --condense listing.txt      (the listing in one line per case: a sha256 over the case's lines; for keeping a comparison's result)

head:  the fused edge head and node head over the cases of tests/test_distance_head_gpu.py and tests/test_node_head_gpu.py (their
       CASES, the bf16 and the full-tile case).  Edge head: per_graph, d_e and the parameter gradients; node head: stats, d_h and the
       parameter gradients (two without LayerNorm).
embed: the edge embedding in both edge dtypes: e, hops and every parameter gradient.  Plain: the shapes of test_edge_embed_vs_oracle
       and test_edge_embed_float_features_vs_oracle (tests/test_model.py), inputs of the tool's own seeds.  Bordered: the shapes,
       graphs and parameters (_embed_inputs with the tests' seeds) of the three bordered embedding tests of
       tests/test_virtual_nodes_gpu.py.  d_e is drawn by the tool in every case.
block: one forward and backward of the fused block / stack through the C ABI: h', e', d_h, d_e and the fourteen parameter gradients
       (per layer) over the block and stack rows of tests/memcontract.py plus BLOCK_EXTRA below; the answer of egt_block_launch_form
       stands next to each row.  The plan's switches are read once per process: run it again under EGT_BWD_MATMUL=bf16x3 (the v5 MM = 1
       instances) and under EGT_NO_NARROW=1 (De = 8 on k_block_bwd_v4r<8>; the static-edge rows are left out there).
ffn:   the channel FFN: y, dx and the six parameter gradients over every (W, matmul, shape, act) of the parametrisations of
       tests/test_ffn_gpu.py (fp32 storage, the tests' seeds), CASES of tests/test_bf16_edges_gpu.py with bf16 storage, and the
       several-tiles-per-wave cases; then, on the cases of test_ffn_bwd_on_a_fresh_workspace_equals_the_prepared_one, egt_ffn_bwd
       on a fresh workspace (flags = 0: it prepares its own operands) next to the autograd path's prepared one.
attn:  the MFMA inner op (d in {16, 32, 64}) forward and backward through the C ABI: v_att, h_hat, rowstats, d_qkv, d_E, d_G over the
       mfma_cases of tests/memcontract.py and the shapes, options and inputs (the tests' seeds) of test_attn_mfma_kernel_vs_oracle,
       test_attn_mfma_in_kernel_random_mask and test_attn_mfma_shared_workspace_fwd_to_bwd (tests/test_attn_gpu.py).  The instance
       choice is read once per process: run it again under EGT_ATTN_GENERIC=1 (the main configuration on the V = 0 instances).
attn_bf16: the same op with bf16 products (desc.reserved = ATTN_WS_SHARED | ATTN_MM_BF16, the workspace of the size query for that
       descriptor) over the same three parametrisations (not the memcontract cases): d in {16, 32, 64}, ragged and odd tile counts, V = 0 / 1 / 2;
       again once more under EGT_ATTN_GENERIC=1.
pair:  the fused pair operator forward and backward through the C ABI: v_att, e_out, rowstats, d_qkv, d_e and the eight parameter
       gradients over the pair_cases of tests/memcontract.py and, in its format, the shapes of
       test_pair_block_in_kernel_random_mask_vs_oracle (tests/test_pair_gpu.py), each with the in-kernel random mask (V = 2) and with
       random_mask_prob = 0 (V = 1)."""
import argparse
import hashlib
import itertools
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(tag, tensors):
    import torch
    for name, t in tensors:
        raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
        print(f"{hashlib.sha256(raw).hexdigest()}  {tag} {name} {str(t.dtype)[6:]}{list(t.shape)}", flush=True)


def condense(path):
    """a listing in one line per case (sha256 over the case's lines, the number of its tensors, its tag) and one for the whole file"""
    import re
    cases, raw = {}, open(path, "rb").read()
    for line in raw.decode().splitlines():
        tag = re.match(r"\w{64}  (.*?) (?:d )?\S+ \w+\[[\d, ]*\]$", line).group(1)
        cases.setdefault(tag, []).append(line)
    for tag, lines in cases.items():
        print(f"{hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}  {len(lines):3d} tensors  {tag}")
    print(f"{hashlib.sha256(raw).hexdigest()}  {len(raw.splitlines())} lines  whole listing")


def params_of(test, names):
    """the values of one pytest.mark.parametrize of `test`, by its argument names"""
    return next(m.args[1] for m in test.pytestmark if m.name == "parametrize" and m.args[0] == names)


def head(gpu):
    import torch
    import test_distance_head_gpu as TD
    import test_node_head_gpu as TN
    from egt_amd.node_head import node_head_loss

    def out_of(out, first, grad_in, names):
        return [(first, out[first]), (grad_in, out[grad_in])] + [("d " + n, g) for n, g in zip(names, out["grads"])]

    edge = [(c, {}) for c in TD.CASES] + [((8, 64, 3, "relu", True), dict(dtype=torch.bfloat16)), ((64, 64, 3, "elu", True), dict(N=16))]
    for case, kw in edge:
        got = TD._run_case(gpu, *case, **kw)[0]
        tag = "edge " + "-".join(map(str, case)) + "".join(f" {k}={str(v).replace('torch.', '')}" for k, v in kw.items())
        emit(tag, out_of(got, "per_graph", "d_e", TD.DR.HEAD_NAMES if case[4] else TD.DR.HEAD_NAMES[2:]))
    for case in TN.CASES:
        x, params, _ = TN._reference(case)
        got, _ = TN._run(node_head_loss, x, params, case[3], gpu)
        emit("node " + "-".join(map(str, case)), out_of(got, "stats", "d_h", TN.NR.NAMES if case[4] else TN.NR.NAMES[2:]))


def embed(gpu):
    import torch
    import test_model as TM
    import test_virtual_nodes_gpu as TV
    from egt_amd import edge_embed

    def plain_inputs(B, N, De, K, V, F):
        g = torch.Generator().manual_seed(B * 100 + N + F)
        adj = (torch.rand(B, N, N, generator=g) > 0.8).float()
        adj = ((adj + adj.transpose(1, 2)) > 0).float()
        fm = torch.where(adj > 0, torch.randint(0, V - 1, (B, N, N), generator=g), torch.tensor(-1)) if V > 1 else torch.full((B, N, N), -1)
        p = dict(table=torch.randn(V, De, generator=g) if V > 1 else torch.zeros(1, De), W=torch.randn(K, De, generator=g) * 0.3,
                 b=torch.randn(De, generator=g) * 0.2)
        ff = None
        if F:
            ff = torch.rand(B, N, N, F, generator=g); ff[adj == 0] = -1.0
            p.update(We=torch.randn(F, De, generator=g), be=torch.randn(De, generator=g) * 0.2)
        return adj, fm, ff, p

    def run(tag, adj, fm, ff, p):
        for edt in ("f32", "bf16"):
            q = {k: v.to(gpu).requires_grad_() for k, v in p.items()}
            kw = {} if ff is None else dict(float_features=ff.to(gpu), float_kernel=q["We"], float_bias=q["be"])
            e, hops = edge_embed(fm.to(gpu), adj.to(gpu), q["table"], q["W"], q["b"], edge_dtype=edt, return_hops=True,
                                 virtual_edge_table=q.get("vn"), **kw)
            de = torch.randn(e.shape, generator=torch.Generator().manual_seed(e.shape[1])).to(e.dtype)
            e.backward(de.to(gpu))
            emit(f"{tag} {edt}", [("e", e), ("hops", hops)] + [("d " + k, v.grad) for k, v in q.items()])

    for B, N, De, K, V in params_of(TM.test_edge_embed_vs_oracle, "B,N,De,K,V"):
        run(f"embed B{B}-N{N}-De{De}-K{K}-V{V}", *plain_inputs(B, N, De, K, V, 0))
    for B, N, De, K, F in params_of(TM.test_edge_embed_float_features_vs_oracle, "B,N,De,K,F"):
        run(f"embed B{B}-N{N}-De{De}-K{K}-F{F}", *plain_inputs(B, N, De, K, 1, F))
    # the bordered tests fix B, N, K (and nv) and the seed of _embed_inputs in their bodies
    fwd = [(2, 19, 4, nv, De, F, nv * 100 + De + F)
           for nv, De, F in params_of(TV.test_bordered_embedding_forward_is_the_plain_one_plus_the_border, "nv,De,F")]
    bwd = [(3, 37, 4, 2, De, 0, De) for De in params_of(TV.test_bordered_embedding_backward, "De")]
    t = TV.test_bordered_backward_is_the_plain_backward_of_the_interior
    walk = [(90, 5, 4, nv, De, F, 1000 + nv * 100 + De + F)
            for nv, De, F in itertools.product(params_of(t, "nv"), params_of(t, "De"), params_of(t, "F"))]
    for B, N, K, nv, De, F, seed in fwd + bwd + walk:
        run(f"embed_vn B{B}-N{N}-De{De}-K{K}-nv{nv}-F{F}", *TV._embed_inputs(B, N, De, K, nv, F, seed=seed))


# block: rows beside the tables of tests/memcontract.py, in their format (no forms claimed: the listing prints what the library answers)
BLOCK_EXTRA = [("n32_de64", 2, 32, 8, 64, False, "", None, None),                  # N a multiple of 16: the non-ragged instances
               ("n32_de32_mask", 2, 32, 8, 32, False, "attn_mask", None, None),
               ("n32_de16", 2, 32, 8, 16, False, "", None, None),
               ("n21_de8", 2, 21, 8, 8, False, "", None, None),                    # k_block_bwd_v4r<8> under EGT_NO_NARROW=1
               ("n90_de64_mask", 1, 90, 8, 64, False, "attn_mask", None, None),    # K/V do not fit in LDS, mask tensor: k_block_fwd<64, false, true, false>
               ("n90_de64", 1, 90, 8, 64, False, "", None, None),                  # ... without one: k_block_fwd<64, false, false, false>
               ("n160_de16", 1, 160, 8, 16, False, "", None, None)]                # k_block_fwd_r4, eight waves, full tiles


def block(gpu):
    import ctypes as C
    import torch
    import memcontract as M
    from egt_amd import _lib as L
    lib = L.load()
    no_narrow = os.environ.get("EGT_NO_NARROW", "") not in ("", "0")       # (the static-edge rows are refused there)
    rows = [(M.block_case, r) for r in M.BLOCK_TABLE + BLOCK_EXTRA if not (no_narrow and "static" in r[6])]
    rows += [(M.stack_case, r) for r in M.STACK_TABLE]
    for make, row in rows:
        case = make(lib, row)
        form = lib.egt_block_launch_form(C.byref(case.claims["desc"])).decode()
        out = M.run(case, M.ZERO, gpu, sync=torch.cuda.synchronize, check_rc=L.check)
        emit(f"block {case.name} [{form}]", sorted(out.items()))


def ffn(gpu):
    import ctypes as C
    import torch
    import test_ffn_gpu as TF
    import test_bf16_edges_gpu as TB
    from egt_amd import _lib as L
    from egt_amd.ffn import _desc, _pstruct
    f32, bf16 = torch.float32, torch.bfloat16

    def run(tag, W, mm, shape, act, seed, dtype=f32):
        m, x, dy, y, dx = TF._ffn_case(shape, act, gpu, seed=seed, W=W, matmul=mm, dtype=dtype)
        tag = f"{tag} W{W}-{mm}-{'x'.join(map(str, shape))}-{act}-{str(dtype)[6:]}"
        emit(tag, [("y", y), ("dx", dx)] + [("d " + n, getattr(m, n).grad) for n in TF.NAMES])
        return m, x, dy, tag

    for W, shape, act in params_of(TF.test_ffn_bf16x3_matmul_holds_the_fp32_tolerances, "W,shape,act"):
        run("ffn", W, "bf16x3", shape, act, W + 1)
    for W, shape in params_of(TF.test_ffn_plain_bf16_matmul, "W,shape"):
        run("ffn", W, "bf16", shape, "elu", W + 2)
    for shape, act in params_of(TF.test_ffn_vs_oracle, "shape,act"):
        run("ffn", 64, "f32", shape, act, 0)
    for W, shape, act in params_of(TF.test_ffn_other_widths_vs_oracle, "W,shape,act"):
        run("ffn", W, "f32", shape, act, W)
    for shape, act in params_of(TF.test_ffn_width8_vs_oracle, "shape,act"):
        run("ffn", 8, "f32", shape, act, 8)
    for W, mm, shape, act in TB.CASES:
        run("ffn_bf16_edges", W, mm, shape, act, W + len(shape), bf16)
    for W, mm, dtype, act in TF.SEVERAL_TILES + [(48, "bf16x3", f32, "relu")]:    # (the last one: relu-step flips keep it out of the test)
        run("ffn_several_tiles", W, mm, (TF.SEVERAL_TILES_ROWS,), act, W + 3, dtype)
    lib = L.load()
    for W, mm in params_of(TF.test_ffn_bwd_on_a_fresh_workspace_equals_the_prepared_one, "W,matmul"):
        m, x, dy, tag = run("ffn_prepared", W, mm, (3, 33, 33), "elu", 11)
        x, dy = x.to(gpu), dy.to(gpu)
        params = [getattr(m, n).detach().contiguous() for n in TF.NAMES]
        desc = _desc(x.numel() // W, W, "elu", 1e-3, mm)
        ws = torch.empty(lib.egt_ffn_workspace_bytes(C.byref(desc)), dtype=torch.uint8, device=gpu)
        dx = torch.empty_like(x)
        grads = [torch.empty_like(p) for p in params]
        pst, gst = _pstruct(params), _pstruct(grads)
        L.check(lib.egt_ffn_bwd(C.byref(desc), C.byref(pst), L.ptr(x), L.ptr(dy), L.ptr(dx), C.byref(gst), L.ptr(ws), L.current_stream()))
        torch.cuda.synchronize()
        emit(tag.replace("ffn_prepared", "ffn_fresh"), [("dx", dx)] + [("d " + n, g) for n, g in zip(TF.NAMES, grads)])


def attn(gpu, bf16=False):
    import ctypes as C
    import torch
    import memcontract as M
    import test_attn_gpu as TA
    from egt_amd import _lib as L
    from egt_amd.functional import AttnConfig, _attn_desc
    lib, H = L.load(), 8
    op = "attn_bf16" if bf16 else "attn"
    for case in [] if bf16 else M.mfma_cases(lib):
        emit(f"attn {case.name}", sorted(M.run(case, M.ZERO, gpu, sync=torch.cuda.synchronize, check_rc=L.check).items()))

    def run(tag, B, N, d, seed, opts, masked, cfg):
        g = torch.Generator().manual_seed(seed)          # the draws in the tests' order
        r = lambda *s: torch.randn(*s, generator=g)
        QKV, E = r(B, N, 3 * d * H) * 0.7, r(B, N, N, H)
        G = r(B, N, N, H) if opts.get("gate", True) else None
        km = None
        if not opts.get("nomask"):
            km = torch.ones(B, N, dtype=torch.uint8); km[masked[0], N - masked[1]:] = 0
        Mt = (torch.rand(B, N, N, generator=g) > 0.4).float()[..., None].repeat(1, 1, 1, H).contiguous() if opts.get("attn_mask") else None
        rm = (torch.rand(B, N, N, H, generator=g) < opts["rand_p"]).to(torch.uint8) if opts.get("rand_p") else None
        dV, dH = r(B, N, d * H), r(B, N, N, H)
        cu = lambda t: None if t is None else t.to(gpu)
        QKV, E, G, km, Mt, rm, dV, dH = map(cu, (QKV, E, G, km, Mt, rm, dV, dH))
        desc = _attn_desc(cfg, B, N, d, True, G is not None, Mt is not None)
        desc.reserved = L.ATTN_WS_SHARED | (L.ATTN_MM_BF16 if bf16 else 0)
        p = C.byref(desc)
        new = lambda *s: torch.zeros(*s, device=gpu)
        v_att, h_hat, rowstats, d_qkv, d_E = new(B, N, d * H), new(B, N, N, H), new(B, N, H, 4), new(B, N, 3 * d * H), new(B, N, N, H)
        d_G = new(B, N, N, H) if G is not None else None
        ws = torch.zeros(lib.egt_attn_mfma_workspace_bytes(p), dtype=torch.uint8, device=gpu)
        common = [L.ptr(t) for t in (QKV, E, G, km, Mt, rm)]
        L.check(lib.egt_attn_mfma_fwd(p, *common, L.ptr(v_att), L.ptr(h_hat), L.ptr(rowstats), L.ptr(ws), L.current_stream()))
        L.check(lib.egt_attn_mfma_bwd(p, *common, L.ptr(v_att), L.ptr(rowstats), L.ptr(dV), L.ptr(dH), L.ptr(d_qkv), L.ptr(d_E), L.ptr(d_G),
                                      L.ptr(ws), L.current_stream()))
        torch.cuda.synchronize()
        emit(tag, [(n, t) for n, t in (("v_att", v_att), ("h_hat", h_hat), ("rowstats", rowstats), ("d_qkv", d_qkv), ("d_E", d_E), ("d_G", d_G))
                   if t is not None])

    for B, N, d, opts in params_of(TA.test_attn_mfma_kernel_vs_oracle, "B,N,d,opts"):
        cfg = AttnConfig(num_heads=H, clip_logits_value=opts.get("clip", (-5.0, 5.0)), random_mask_prob=0.5 if opts.get("rand_p") else 0.0,
                         training=bool(opts.get("rand_p")), need_a_tild=False)
        run(f"{op} vs_oracle B{B}-N{N}-d{d}-{'-'.join(f'{k}={v}' for k, v in opts.items()) or 'main'}", B, N, d, B * 100 + N + d, opts, (0, 5), cfg)
    for N, d in params_of(TA.test_attn_mfma_in_kernel_random_mask, "N,d"):
        run(f"{op} in_kernel_random_mask N{N}-d{d}", 2, N, d, N + d, {}, (1, 7),
            AttnConfig(num_heads=H, random_mask_prob=0.25, training=True, seed=4242, need_a_tild=False))
    for N, d in params_of(TA.test_attn_mfma_shared_workspace_fwd_to_bwd, "N,d"):
        run(f"{op} shared_workspace N{N}-d{d}", 2, N, d, N * 3 + d, {}, (1, 7), AttnConfig(num_heads=H, need_a_tild=False))


def pair(gpu):
    import torch
    import memcontract as M
    import test_pair_gpu as TP
    from egt_amd import _lib as L
    lib = L.load()
    cases = [(c, 2) for c in M.pair_cases(lib)]
    for B, N, nodes in params_of(TP.test_pair_block_in_kernel_random_mask_vs_oracle, "B,N,nodes"):
        for v in (2, 1):
            case = M.pair_case(lib, B, N, nodes[-1], True)
            if v == 1:
                case.claims["desc"].random_mask_prob = 0.0      # (the steps hold the descriptor by reference) no in-kernel random mask
            cases.append((case, v))
    for case, v in cases:
        emit(f"pair {case.name} V{v}", sorted(M.run(case, M.ZERO, gpu, sync=torch.cuda.synchronize, check_rc=L.check).items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--ops", default="head,embed")
    ap.add_argument("--condense", default=None, metavar="LISTING", help="print a saved listing in one line per case (no GPU work)")
    args = ap.parse_args()
    if args.condense:
        return condense(args.condense)
    ops = args.ops.split(",")
    if not ops or set(ops) - {"head", "embed", "block", "ffn", "attn", "attn_bf16", "pair"}:
        ap.error("--ops takes head, embed, block, ffn, attn, attn_bf16, pair or several of them")
    if args.lib:
        os.environ["EGT_AMD_LIB"] = os.path.abspath(args.lib)      # read when egt_amd._lib is imported
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import torch
    gpu = torch.device("cuda", 0)
    for op, fn in (("head", head), ("embed", embed), ("block", block), ("ffn", ffn), ("attn", attn), ("attn_bf16", lambda g: attn(g, bf16=True)),
                   ("pair", pair)):
        if op in ops:
            fn(gpu)


if __name__ == "__main__":
    main()
