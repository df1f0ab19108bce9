#!/usr/bin/env python3
"""Where the error of h' sits in a conditioning case of the cross-talk FFN (tests/conditioning.py, operator `xtalk`):

    python tools/xtalk_node_side.py            (one GPU, a few seconds; run from the repository root)

Per (case, recipe): the margins of the fused op under conditioning.compare, the composed route's h' update, then the node side
piece by piece against fp64 -- torch's layer_norm of h, fnn_lr1_node (from the GPU's and from the fp64 LayerNorm), hn out of
egt_xtalk_fwd -- and the h' update recomputed with each of (xn, hn) replaced by its fp64 value.  Margins are |error| / util.FWD.
DESIGN.md section 7 item 10 quotes a run."""
import os
import sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch, torch.nn.functional as F
import conditioning as CD, xtalk_cases as XC
from oracle import egt_oracle as O
from util import FWD, margin
from egt_amd import xtalk as XT
dev = torch.device("cuda:0")
NAMES = CD.FFN_NAMES


def m(a, r, scale_ref=None):
    a, r = a.detach().double().cpu(), r.detach().double().cpu()
    s = r if scale_ref is None else scale_ref.detach().double().cpu()
    tol = FWD["arel"] * float(s.abs().max()) + FWD["rtol"] * r.abs()
    return float(((a - r).abs() / tol).max())


for cid, recipe in (("n37_de64", "plain"), ("n37_de64", "const_rows"), ("n37_de64", "offset32"), ("n21_de64_sn64", "const_rows"),
                    ("n9_de16", "const_rows"), ("n19_de32_relu", "const_rows"), ("n33_de16_empty", "const_rows")):
    case = CD.make_xtalk(cid, recipe)
    c, inp = case["c"], case["inp"]
    ref = CD.xtalk_oracle(case)
    sink = {}
    CD.compare(CD.xtalk_gpu(case, dev), ref, case, check=False, sink=sink)
    print(f"== {cid} {recipe} Dh {c['Dh']} act {c['act']}: fused", {k: round(v, 4) for k, v in sink.items() if v > 0.03 or k in ("h_out", "e_out")})
    # composed (all torch) route
    h, e = inp["h"].to(dev), inp["e"].to(dev)
    p = {k: v.to(dev) for k, v in case["params"].items()}
    pn = [p[f"node.{k}"] for k in NAMES]; pe = [p[f"edge.{k}"] for k in NAMES]
    h2c, e2c = XT.xtalk_ffn_composed(h, e, inp["mask"].to(dev), pn, pe, c["n2e"], c["e2n"], c["act"])
    hd = inp["h"].double()
    print("   composed h_out update margin", round(m(h2c.cpu().double() - hd, ref["h_out"] - hd), 4))
    # pieces in fp64
    p64 = {k: v.double() for k, v in case["params"].items()}
    pn64 = {k: p64[f"node.{k}"] for k in NAMES}; pe64 = {k: p64[f"edge.{k}"] for k in NAMES}
    s_e, s_n, _, _ = XC.widths(c["De"], c["Dh"], c["n2e"], c["e2n"])
    ln64 = O.layer_norm(hd, pn64["norm_gamma"], pn64["norm_beta"])
    xn64 = O.dense(ln64, pn64["lr1_kernel"], pn64["lr1_bias"])
    hr64, hc64 = xn64[..., :s_n], xn64[..., s_n:2 * s_n]
    _, hn64 = XC.xtalk_edge_ref(inp["e"].double(), inp["mask"], hr64, hc64, pe64, s_e, s_n, c["act"])
    # GPU pieces
    ln = F.layer_norm(h, (c["Dh"],), pn[0], pn[1], XT.LN_EPS)
    xn = XT._dense(ln, pn[2], pn[3])
    print("   LN(h) gpu margin", round(m(ln, ln64), 4), " xn gpu margin", round(m(xn, xn64), 4),
          " xn from fp64 LN by gpu addmm", round(m(XT._dense(ln64.float().to(dev), pn[2], pn[3]), xn64), 4))
    hr, hc = xn[..., :s_n].contiguous(), xn[..., s_n:2 * s_n].contiguous()
    desc = XT._desc(c["B"], c["N"], c["De"], c["Dh"], s_e, s_n, c["act"])
    e2, hn = XT._XtalkEdge.apply(e, inp["mask"].to(dev).float(), hr, hc, desc, *pe)
    print("   hn gpu margin", round(m(hn, hn64), 4))
    act = (lambda t: F.elu(t)) if c["act"] == "elu" else torch.relu
    upd64 = ref["h_out"] - hd
    for tag, xt_, hn_ in (("xn gpu, hn gpu", xn, hn), ("xn fp64, hn gpu", xn64.float().to(dev), hn), ("xn gpu, hn fp64", xn, hn64.float().to(dev)),
                          ("xn fp64, hn fp64 (gpu lr2 only)", xn64.float().to(dev), hn64.float().to(dev))):
        z = torch.cat([xt_[..., 2 * s_n:], hn_], dim=-1)
        upd = XT._dense(act(z), pn[4], pn[5])
        stored = (h + upd).cpu().double() - hd
        print(f"   h update [{tag}]: as computed {m(upd, upd64):.4f}, after h + upd stored in fp32 {m(stored, upd64):.4f}")
    print("   max|h|", float(h.abs().max()), "max|upd|", float(upd64.abs().max()))
