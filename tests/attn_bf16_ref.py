"""Reference side of the MFMA inner op's bf16-product mode (EGT_ATTN_MM_BF16, AttnConfig(matmul="bf16")):
  * the case table of tests/test_attn_bf16_gpu.py (shared with the CPU fairness cap);
  * rounded_inputs: the oracle's inputs with the four operand tensors of the contract rounded (the oracle then differs from the
    kernels by the two IN-FLIGHT roundings only: the probabilities P and the logit gradient dS);
  * emulate: an fp64 restatement of the contract with all six rounding points (include/egt_amd.h), forward and backward by hand.
With round=False the emulation is the plain operator: tests/test_attn_bf16_cpu.py checks it against the autograd oracle, so the
hand-written backward is pinned before it is used as evidence."""
import torch

import cases as CS
from oracle import egt_oracle as O

# Half of BF16_TOL elementwise (tests/test_ffn_gpu.py), three times the emulated normalised L2 error (1.6-1.7e-3: two
# independent roundings of rms 2^-9 / sqrt(3) per product term).  The factor covers what the emulation cannot reproduce: P rounded
# relative to the running maximum of the online softmax, fp32 accumulation order, rounding ties.
ATTN_BF16_TOL = dict(rtol=1e-2, arel=5e-3, l2=5e-3)
BF16_TOL = dict(rtol=2e-2, arel=1e-2, l2=2e-2)   # the outer contract (plain bf16 products)

# name -> (B, N, d, options); options as in tests/test_attn_gpu.py::test_attn_mfma_kernel_vs_oracle
CASES = {
    "n48_d64": (2, 48, 64, {}),
    "n37_d16": (2, 37, 16, {}),
    "n21_d32": (2, 21, 32, {}),                                   # s = 32^-1/2 is not a power of two
    "n16_d16_randmask": (2, 16, 16, dict(rand_p=0.3)),            # injected random mask
    "n33_d64_noclip_nomask": (1, 33, 64, dict(clip=None, nomask=True)),
    "n21_d32_ungated": (2, 21, 32, dict(gate=False)),
    "n24_d16_attn_mask": (2, 24, 16, dict(attn_mask=True)),
    "n17_d64": (1, 17, 64, {}),                                   # one full and one ragged tile
    "n128_d64": (1, 128, 64, {}),                                 # several workgroups per graph
}
RNG_CASES = {"rng_n48_d64": (2, 48, 64), "rng_n37_d16": (2, 37, 16)}   # in-kernel random mask: (B, N, d)
RNG_SEED, RNG_P = 4242, 0.25
H = 8


def make_case(name):
    """(inp, attrs) of CASES[name]: fp32 inputs as the kernels see them"""
    B, N, d, opts = CASES[name]
    g = torch.Generator().manual_seed(B * 100 + N + d + 7)
    QKV = torch.randn(B, N, 3 * d * H, generator=g) * 0.7
    E = torch.randn(B, N, N, H, generator=g)
    G = torch.randn(B, N, N, H, generator=g) if opts.get("gate", True) else None
    mask = None
    if not opts.get("nomask"):
        mask = torch.ones(B, N, dtype=torch.bool); mask[0, N - 5:] = False
    M = None
    if opts.get("attn_mask"):
        M = (torch.rand(B, N, N, generator=g) > 0.4).float()[..., None].repeat(1, 1, 1, H).contiguous()
    rm = (torch.rand(B, N, N, H, generator=g) < opts["rand_p"]) if opts.get("rand_p") else None
    dV = torch.randn(B, N, d * H, generator=g); dH = torch.randn(B, N, N, H, generator=g)
    inp = dict(QKV=QKV, E=E, G=G, M=M, mask=mask, rand_mask=rm, drop_keep=None, dV=dV, dH=dH)
    attrs = dict(num_heads=H, clip_logits_value=opts.get("clip", (-5.0, 5.0)), scale_degree=False, scaler_type="log",
                 num_virtual_nodes=0, attn_dropout=0.0)
    return inp, attrs


def make_rng_case(name, rand_mask):
    """(inp, attrs) of RNG_CASES[name]; rand_mask: the bytes of the in-kernel stream (mask_sample on the GPU, rng_ref on the CPU)"""
    B, N, d = RNG_CASES[name]
    g = torch.Generator().manual_seed(N + d + 11)
    QKV = torch.randn(B, N, 3 * d * H, generator=g) * 0.7
    E = torch.randn(B, N, N, H, generator=g); G = torch.randn(B, N, N, H, generator=g)
    mask = torch.ones(B, N, dtype=torch.bool); mask[1, N - 7:] = False
    dV = torch.randn(B, N, d * H, generator=g); dH = torch.randn(B, N, N, H, generator=g)
    inp = dict(QKV=QKV, E=E, G=G, M=None, mask=mask, rand_mask=rand_mask, drop_keep=None, dV=dV, dH=dH)
    attrs = dict(num_heads=H, clip_logits_value=(-5.0, 5.0), scale_degree=False, scaler_type="log", num_virtual_nodes=0,
                 attn_dropout=0.0)
    return inp, attrs


def bf16(t):
    """round to nearest even to bfloat16, returned in t's dtype (t is fp32-representable or is rounded to fp32 first)"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _scale32(d):
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(d), dtype=torch.float32)))


def _split_rounded(QKV, d):
    """(bf16(fl32(s Q)), bf16(K), bf16(V)) as fp64 [B,N,d,H]; s = fl32(d^-1/2) as the library computes it"""
    B, N, _ = QKV.shape
    Q, K, V = QKV.to(torch.float32).reshape(B, N, 3, d, H).unbind(2)
    Qs = bf16(Q * torch.tensor(_scale32(d), dtype=torch.float32))
    return Qs.double(), bf16(K).double(), bf16(V).double()


def rounded_inputs(inp, d):
    """the oracle's inputs for the bf16 mode: bf16(fl32(s Q)) / s, bf16(K), bf16(V), bf16(dV) (fp64 tensors: Q / s is not an fp32
    value in general; the oracle multiplies by s again)"""
    Qs, Kb, Vb = _split_rounded(inp["QKV"], d)
    B, N = inp["QKV"].shape[:2]
    out = dict(inp)
    out["QKV"] = torch.stack([Qs / (d ** -0.5), Kb, Vb], dim=2).reshape(B, N, 3 * d * H)
    out["dV"] = bf16(inp["dV"]).double()
    return out


def emulate(inp, attrs, d, round=True):
    """fp64 evaluation of the contract.  round=True: the six rounding points; round=False: the plain operator (what the autograd
    oracle computes).  Returns V_att, H_hat, dQKV, dE, dG like cases.attn_oracle."""
    rd = bf16 if round else (lambda t: t)
    f64 = lambda t: None if t is None else t.double()
    B, N, _ = inp["QKV"].shape
    s = d ** -0.5
    if round:
        Qs, Kb, Vb = _split_rounded(inp["QKV"], d)
    else:
        Q, K, V = f64(inp["QKV"]).reshape(B, N, 3, d, H).unbind(2)
        Qs, Kb, Vb = Q * s, K, V
    E, G, M = f64(inp["E"]), f64(inp["G"]), f64(inp["M"])
    dO_full = f64(inp["dV"]).reshape(B, N, d, H)
    dO = rd(dO_full)
    dH_ext = f64(inp["dH"])
    clip = attrs["clip_logits_value"]

    raw = torch.einsum("bldh,bmdh->blmh", Qs, Kb)
    A_hat = raw if clip is None else torch.clamp(raw, clip[0], clip[1])
    H_hat = A_hat if E is None else A_hat + E
    x = H_hat
    Gx = G
    adds = []
    if inp["mask"] is not None:
        adds.append((inp["mask"][:, None, :, None].double() - 1) * O.NEG)
    if M is not None:
        adds.append((M - 1) * O.NEG)
    if inp["rand_mask"] is not None:
        adds.append(torch.where(inp["rand_mask"], torch.tensor(-O.NEG, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64)))
    for a in adds:
        x = O._add_mask(x, a)
        if G is not None:
            Gx = O._add_mask(Gx, a)
    S = torch.softmax(x, dim=2)
    g = torch.sigmoid(Gx) if G is not None else torch.ones_like(S)
    P = S * g
    Ov = torch.einsum("blmh,bmdh->bldh", rd(P), Vb)                  # V_att [B,N,d,H]

    dP = torch.einsum("bldh,bmdh->blmh", dO, Vb)                      # dA: bf16 x bf16 products, exact in fp32
    delta = (dO_full * Ov).sum(dim=2)[:, :, None, :]                 # sum_k dO O from the unrounded dO
    dHh = S * (dP * g - delta) + dH_ext
    dS = dHh if clip is None else torch.where((raw < clip[0]) | (raw > clip[1]), torch.zeros_like(dHh), dHh)
    dSb = rd(dS)
    dVg = torch.einsum("blmh,bldh->bmdh", rd(P), dO)
    dK = torch.einsum("blmh,bldh->bmdh", dSb, Qs)
    dQ = torch.einsum("blmh,bmdh->bldh", dSb, Kb) * s
    out = dict(V_att=Ov.reshape(B, N, d * H), H_hat=H_hat, dQKV=torch.stack([dQ, dK, dVg], dim=2).reshape(B, N, 3 * d * H))
    out["dE"] = dHh if E is not None else None
    out["dG"] = dP * S * g * (1 - g) if G is not None else None
    return out


def oracle_rounded(inp, attrs, d):
    return CS.attn_oracle(rounded_inputs(inp, d), attrs)
