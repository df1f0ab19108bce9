"""The launch plane of the cross-talk FFN's edge side (csrc/egt_xtalk.hip: plan_xtalk, the fifteen <W, SNT> instances per
direction) as case tables, a Python restatement of the plan, an fp64 reference of egt_xtalk_fwd / egt_xtalk_bwd and a
comparison that the residual cannot loosen.

A ROW is (B, N, De, Dh, s_e, s_n, activation or None, nodes).  `nodes` holds one entry per graph: an int n is a prefix mask of
n real nodes, "holes" keeps i % 3 != 1, "last" keeps only index N - 1.  The activation alternates elu / relu with the row's
index in its table unless the row names one (row_act).  The operator is called through _XtalkEdge with a descriptor built from
s_e and s_n themselves, so the split positions are free of the fractions' rounding (xtalk.split_widths).

    INSTANCES  every <W, SNT>, W in {16, 32, 64} x SNT in 0..4, each with a partial last exchange tile and an er / ec boundary
               inside a 16-channel tile with ec crossing a tile boundary (s_e = 12 / 20 / 36)
    SPLITS     s_e in {0, 4, W - 4, W} per W (s_e = W: fnn_lr2_edge reads only the exchange), s_n = 4 and s_n = Dh = 48
    SIZES      N = 1 .. 150: below one row block, exact multiples of 8 / 16, one past them, the workload's N = 64, up to five
               workgroups per graph (N = 150: 19 row blocks, the last workgroup with one idle wave), an empty second graph (N = 1)
    GROWTH     B large enough that plan_xtalk grows the backward's rows per wave past 8 (XT_BWD_WG_CAP = 512)
    MASKS      one graph each of: fully real, interior holes, a single real node at the last index, empty

`hold` compares e' as its UPDATE e' - e (both in fp64: tests/conditioning.py explains why the whole e' lets the update hide
behind the residual) and hn under util.FWD; d_e, d_hr, d_hc and the six parameter gradients under util.BWD, with BWD's zero_atol
where max|ref| < 1e-9.  Tensors that do not exist (hn with s_e = 0, d_hr / d_hc with s_n = 0) are absent on both sides.

No test functions here."""
from __future__ import annotations

import collections
import zlib

import torch

import xtalk_cases as XC
from util import FWD, BWD, assert_close, margin

F64 = torch.float64
NAMES = XC.FFN_NAMES
XT_BWD_WG_CAP = 512

Plan = collections.namedtuple("Plan", "W snt rb_f nblk_f wpg_f rb_b nblk_b wpg_b total walk2")


def _al(n):
    return (n + 63) // 64 * 64


def plan(B, N, De, s_e, s_n):
    """plan_xtalk restated: rows per wave, row blocks and workgroups per graph of both directions, workspace floats"""
    W, snt = De, (s_n + 15) // 16
    kt = 2 * (W // 16) + snt
    s1f, s2f = 2 * W * W, kt * 16 * W
    part_len = s1f + s2f + 3 * W
    rb_f = 8
    nblk_f = -(-N // rb_f)
    wpg_f = -(-nblk_f // 4)
    rb_b = 8
    while True:
        nblk_b = -(-N // rb_b)
        wpg_b = -(-nblk_b // 4)
        if B * wpg_b <= XT_BWD_WG_CAP or rb_b >= N:
            break
        rb_b += 8
    total = 2 * s1f + 2 * s2f + _al(2 * W) + _al(part_len) + _al(B * N * s_e) + _al(B * nblk_f * N * max(s_e, s_n)) \
        + B * wpg_b * part_len
    return Plan(W, snt, rb_f, nblk_f, wpg_f, rb_b, nblk_b, wpg_b, total, W == 64 and snt >= 3)


def launch_form(B, N, De, s_e, s_n):
    """what egt_xtalk_launch_form answers for the plan above"""
    p = plan(B, N, De, s_e, s_n)
    return (f"fwd=k_xtalk_fwd<{p.W},{p.snt}>/rb{p.rb_f}/g{B * p.wpg_f} "
            f"bwd=k_xtalk_bwd<{p.W},{p.snt}>/rb{p.rb_b}/g{B * p.wpg_b}{'/walk2' if p.walk2 else ''}")


# ------------------------------------------------------------------------------------------------------- tables -----
_SE = {16: 12, 32: 20, 64: 36}
INSTANCES = [(2, 19, W, 64, _SE[W], s_n, None, (19, 11)) for W in (16, 32, 64) for s_n in (0, 12, 20, 36, 52)]

SPLITS = [(2, 19, W, 64, s_e, 16, None, (19, 11)) for W in (16, 32, 64) for s_e in (0, 4, W - 4, W)] + \
         [(2, 19, 32, 48, 8, s_n, None, (19, 11)) for s_n in (4, 48)]

SIZES = [(2, N, 16, 64, 4, 16, None, (N, max(0, N - 5))) for N in (1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 150)] + \
        [(2, 64, 64, 64, 16, 16, None, (64, 40)),
         (1, 65, 64, 64, 16, 32, None, (58,))]          # instance <64,2>: nine row blocks in three workgroups


def _cycling(B, N):
    return tuple(N - (3 * b) % N for b in range(B))


# fp64 reference on one CPU thread, chunked over graphs: (257, 37) 1.0 s, (513, 19) 0.5 s, (200, 65) 2.7 s (fp32: 1.0 s)
GROWTH = [(B, N, 16, 64, 4, 16, None, _cycling(B, N)) for B, N in ((257, 37), (513, 19), (200, 65))]

MASKS = [(4, 21, 32, 64, 8, 16, None, (21, "holes", "last", 0))]

TABLES = dict(INSTANCES=INSTANCES, SPLITS=SPLITS, SIZES=SIZES, GROWTH=GROWTH, MASKS=MASKS)
TWICE = GROWTH + [SIZES[-1]]       # also run twice and compared bit for bit


def all_rows():
    return [(t, i, row) for t, rows in TABLES.items() for i, row in enumerate(rows)]


def row_id(table, i, row):
    B, N, De, Dh, s_e, s_n = row[:6]
    return f"{table}{i}-B{B}_N{N}_De{De}_Dh{Dh}_se{s_e}_sn{s_n}_{row_act(table, i, row)}"


def row_act(table, i, row):
    return row[6] or ("elu", "relu")[i % 2]


def row_mask(row):
    B, N, nodes = row[0], row[1], row[7]
    idx = torch.arange(N)
    m = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate(nodes):
        m[b] = {"holes": idx % 3 != 1, "last": idx == N - 1}[n] if isinstance(n, str) else idx < n
    return m


# -------------------------------------------------------------------------------------------- inputs, reference -----
def edge_inputs(row):
    """-> ({e, mask, hr, hc, d_e_out, d_hn}, edge parameters): fp32 tensors of a seeded recipe; hr / hc are None with s_n = 0,
    d_hn with s_e = 0"""
    B, N, De, Dh, s_e, s_n = row[:6]
    g = torch.Generator().manual_seed(zlib.crc32(repr(row).encode()) & 0x7FFFFFFF)
    r = lambda *s: torch.randn(*s, generator=g)
    inp = dict(e=r(B, N, N, De) * 1.5 + 0.2, mask=row_mask(row), hr=r(B, N, s_n) * 0.8 if s_n else None,
               hc=r(B, N, s_n) * 0.8 if s_n else None, d_e_out=r(B, N, N, De), d_hn=r(B, N, s_e) if s_e else None)
    return inp, XC.ffn_params(De, 2 * De - 2 * s_e + s_n, g)


def _reference(row, act, dtype, pairs_per_chunk=1 << 17):
    """XC.xtalk_edge_ref in `dtype` over chunks of graphs (graphs are independent; the parameter gradients add)"""
    B, N, De, Dh, s_e, s_n = row[:6]
    inp, pe = edge_inputs(row)
    p = {k: v.to(dtype).requires_grad_() for k, v in pe.items()}
    step = max(1, pairs_per_chunk // (N * N))
    outs = collections.defaultdict(list)
    pg = None
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        e = inp["e"][sl].to(dtype).requires_grad_()
        leaves = [e]
        hr = hc = None
        if s_n:
            hr, hc = inp["hr"][sl].to(dtype).requires_grad_(), inp["hc"][sl].to(dtype).requires_grad_()
            leaves += [hr, hc]
        e2, hn = XC.xtalk_edge_ref(e, inp["mask"][sl], hr, hc, p, s_e, s_n, act)
        loss = (e2 * inp["d_e_out"][sl].to(dtype)).sum()
        if s_e:
            loss = loss + (hn * inp["d_hn"][sl].to(dtype)).sum()
        gr = torch.autograd.grad(loss, leaves + [p[k] for k in NAMES])
        outs["e_out"].append(e2.detach())
        outs["d_e"].append(gr[0])
        if s_e:
            outs["hn"].append(hn.detach())
        if s_n:
            outs["d_hr"].append(gr[1]); outs["d_hc"].append(gr[2])
        tail = gr[len(leaves):]
        pg = list(tail) if pg is None else [a + b for a, b in zip(pg, tail)]
    out = {k: torch.cat(v) for k, v in outs.items()}
    out.update({"edge." + k: t for k, t in zip(NAMES, pg)})
    return out


def edge_reference(row, act):
    """fp64: e', hn and the gradients of sum(e' d_e_out) + sum(hn d_hn) w.r.t. e, hr, hc and the six parameters.  Not cached:
    each test file uses a row's reference once, and the GROWTH rows' outputs are ~100 MB each."""
    return _reference(row, act, F64)


def edge_oracle_fp32(row, act):
    """the same reference code in fp32 (the fairness condition of tests/test_xtalk_plane_cpu.py)"""
    return _reference(row, act, torch.float32)


def desc(row, act):
    from egt_amd.xtalk import _desc
    B, N, De, Dh, s_e, s_n = row[:6]
    return _desc(B, N, De, Dh, s_e, s_n, act)


def _nan_tailed(t, dev):
    """t on the device as the head of a buffer whose 16 floats past the end are NaN: a partial exchange tile read past s_n
    (xt_node4's k < sn) meets zero weights and would otherwise leave no trace in any result.
    The limit of this: only a read past s_n on the LAST (b, n) row reaches the NaNs; on every other row it lands in the next row's
    finite values, times zero weights, and stays invisible.  It also needs the operator to take the view as it is (a contiguous
    fp32 view is not copied by _f32c), which the data_ptr assertion in edge_gpu holds."""
    buf = torch.full((t.numel() + 16,), float("nan"), device=dev)
    v = buf[:t.numel()].view(t.shape)
    v.copy_(t)
    return v.requires_grad_()


def edge_gpu(row, act, dev):
    """one egt_xtalk_fwd + egt_xtalk_bwd through _XtalkEdge on the row's fp32 tensors -> the reference's names"""
    from egt_amd.xtalk import _XtalkEdge
    s_e, s_n = row[4], row[5]
    inp, pe = edge_inputs(row)
    e = inp["e"].to(dev).requires_grad_()
    hr = hc = None
    if s_n:
        hr, hc = _nan_tailed(inp["hr"], dev), _nan_tailed(inp["hc"], dev)
        assert all(t.contiguous().data_ptr() == t.data_ptr() for t in (hr, hc))      # the kernel reads the buffer with the NaN tail
    ps = [pe[k].to(dev).requires_grad_() for k in NAMES]
    e2, hn = _XtalkEdge.apply(e, inp["mask"].to(dev).float(), hr, hc, desc(row, act), *ps)
    outs, ups = [e2], [inp["d_e_out"].to(dev)]
    if s_e:
        outs.append(hn); ups.append(inp["d_hn"].to(dev))
    torch.autograd.backward(outs, ups)
    out = dict(e_out=e2.detach(), d_e=e.grad)
    if s_e:
        out["hn"] = hn.detach()
    if s_n:
        out["d_hr"], out["d_hc"] = hr.grad, hc.grad
    out.update({"edge." + k: t.grad for k, t in zip(NAMES, ps)})
    return out


# --------------------------------------------------------------------------------------------------- comparison -----
def hold(got, ref, e, *, check=True, sink=None, name=""):
    """`got` against the fp64 `ref` (e: the row's input, the base of the update).  check=True asserts util.FWD / util.BWD;
    returns the worst margin and adds each tensor's to `sink`."""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    base = e.detach().double().cpu()
    worst = 0.0
    for k, r in ref.items():
        fwd = k in ("e_out", "hn")
        tol = FWD if fwd else BWD
        a, r = got[k].detach().double().cpu(), r.detach().double().cpu()
        assert a.shape == r.shape, f"{name} {k}: shape {tuple(a.shape)} vs {tuple(r.shape)}"
        label = k
        if k == "e_out":
            a, r, label = a - base, r - base, "e_out (update)"
        if not fwd and float(r.abs().max()) < 1e-9:
            m = float((a - r).abs().max()) / BWD["zero_atol"]
        else:
            m = margin(a, r, rtol=tol["rtol"], arel=tol["arel"])
        worst = max(worst, m)
        if sink is not None:
            sink[label] = max(sink.get(label, 0.0), m)
        if check:
            assert_close(a, r, name=f"{name} {label}", **tol)
    return worst
