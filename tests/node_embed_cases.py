"""Case table of the node-input embedding (egt_amd/node_embed.py, egt_node_embed_*): the smallest shapes at which each thing
can go wrong, host inputs, and the fp64 oracle (oracle/egt_model_oracle.py: neg1_masked_embedding, keras_masking,
svd_embedding / eig_embedding; the virtual rows are VNModel.combine_node_embeddings, graph_model_base.py:227-235).  No test
functions here: tests/test_node_embed_cpu.py admits the table, tests/test_node_embed_gpu.py runs it."""
from __future__ import annotations

import zlib

import torch

# id -> B, N, Dh, nv, R (integer kind) or F (float kind), pe (kind, sel, T, transform) or None, counts (real nodes per graph)
CASES = {
    "lookup": dict(B=2, N=9, Dh=64, nv=0, R=29),
    "w48_eig": dict(B=1, N=37, Dh=48, nv=0, R=29, pe=("eig", 8, 20, False)),
    "empty_n65_vn1_svd": dict(B=3, N=65, Dh=64, nv=1, R=29, pe=("svd", 8, 16, True), counts=[65, 0, 17]),
    "pattern_eig2": dict(B=5, N=20, Dh=64, nv=0, R=4, pe=("eig", 2, 20, False)),
    "cluster_eig20": dict(B=2, N=23, Dh=64, nv=0, R=8, pe=("eig", 20, 20, False)),
    "w16_nv2": dict(B=2, N=7, Dh=16, nv=2, R=29),
    "w32_nv16": dict(B=1, N=5, Dh=32, nv=16, R=29),
    "float5_svd_nv0": dict(B=2, N=21, Dh=64, nv=0, F=5, pe=("svd", 8, 16, True)),
    "float5_svd_nv1": dict(B=2, N=21, Dh=64, nv=1, F=5, pe=("svd", 8, 16, True)),
    "float3": dict(B=2, N=12, Dh=64, nv=0, F=3),
    "svd_notransform": dict(B=2, N=11, Dh=64, nv=0, R=29, pe=("svd", 8, 16, False)),
    "eig_transform": dict(B=2, N=11, Dh=64, nv=0, R=29, pe=("eig", 8, 20, True)),
    "b37_n40_svd_vn1": dict(B=37, N=40, Dh=64, nv=1, R=29, pe=("svd", 8, 16, True)),
}
PARAMS = ("node_emb", "node_emb_bias", "pe_kernel", "pe_bias", "virtual_node_emb")
_CACHE = {}


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def sign_width(c):
    """signs per graph as the model draws them: the untransformed encoding is zero-padded before the flip"""
    kind, sel, _, transform = c["pe"]
    return sel if transform else max(sel, c["Dh"] // 2 if kind == "svd" else c["Dh"])


def make(name):
    """host tensors of a case (fp32 / int32), built once: features, pe, signs (the model's shape), params {name: tensor or
    None}, d_h (mixed signs) and d_h_pos (all positive: a dropped partial sum cannot cancel)"""
    if name in _CACHE:
        return _CACHE[name]
    c = dict(CASES[name])
    c.setdefault("pe", None)
    g = _gen(name)
    B, N, Dh, nv = c["B"], c["N"], c["Dh"], c["nv"]
    counts = c.get("counts") or [max(1, N - (3 * b + 2) % max(1, N // 2)) for b in range(B)]
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    real = torch.arange(N)[None, :] < torch.tensor(counts)[:, None]
    p = dict.fromkeys(PARAMS)
    if "R" in c:
        feat = torch.randint(0, c["R"] - 1, (B, N), generator=g, dtype=torch.int32)
        feat[~real] = -1
        p["node_emb"] = torch.empty(c["R"], Dh).uniform_(-0.05, 0.05, generator=g)
    else:
        feat = r(B, N, c["F"])
        feat[:, 0, 1] = -1.0                       # one feature at the mask value does not mask the row
        feat[~real] = -1.0
        p["node_emb"] = r(c["F"], Dh) * 0.3
        p["node_emb_bias"] = r(Dh) * 0.2
    pe = signs = None
    if c["pe"]:
        kind, sel, T, transform = c["pe"]
        pe = r(B, N, T, 2) if kind == "svd" else r(B, N, T)
        pe[~real] = 0.0                            # the collate pads the encoding with zeros
        w = sign_width(c)
        signs = torch.where(torch.rand(B, 1, w, generator=g) < 0.5, -1.0, 1.0)
        if kind == "svd":
            signs = signs[..., None]
        if transform:
            p["pe_kernel"] = r((2 if kind == "svd" else 1) * sel, Dh) * 0.3
            p["pe_bias"] = r(Dh) * 0.2
    if nv:
        p["virtual_node_emb"] = torch.empty(nv, Dh).uniform_(-0.05, 0.05, generator=g)
    d_h = r(B, nv + N, Dh)
    c.update(name=name, features=feat, pe_t=pe, signs=signs, params=p, d_h=d_h, d_h_pos=d_h.abs() + 0.1, counts=counts)
    _CACHE[name] = c
    return c


def args(c, dtype=torch.float32, device="cpu", signs=True, leaf=True):
    """(positional args of node_embed / node_embed_composed, the parameter leaves in PARAMS order)"""
    mk = lambda t: None if t is None else t.to(device=device, dtype=dtype).requires_grad_(leaf)
    p = {k: mk(v) for k, v in c["params"].items()}
    kind, sel = (c["pe"][0], c["pe"][1]) if c["pe"] else (None, 0)
    feat = c["features"].to(device)
    if feat.dtype.is_floating_point:
        feat = feat.to(dtype)
    pe = None if c["pe_t"] is None else c["pe_t"].to(device=device, dtype=dtype)
    sg = c["signs"].to(device=device, dtype=dtype) if (signs and c["signs"] is not None) else None
    dense = (p["pe_kernel"], p["pe_bias"]) if p["pe_kernel"] is not None else None
    return (feat, p["node_emb"], p["node_emb_bias"], pe, kind, sel, dense, sg, p["virtual_node_emb"], -1.0), p


def grads(h, p, d_h):
    names = [k for k in PARAMS if p[k] is not None]
    gs = torch.autograd.grad((h * d_h.to(h.dtype).to(h.device)).sum(), [p[k] for k in names], retain_graph=True)
    return dict(zip(names, gs))


def oracle(c, signs=True, dtype=torch.float64):
    """(h, mask, {param: gradient for d_h}, {param: gradient for d_h_pos}) from the oracle's statements, in `dtype`"""
    key = (c["name"], signs, dtype)
    if key in _CACHE:
        return _CACHE[key]
    from oracle import egt_model_oracle as M
    from oracle import egt_oracle as O
    (feat, _, _, pe, kind, sel, _, sg, _, mv), p = args(c, dtype, signs=signs)
    if feat.dtype.is_floating_point:
        x, mask = M.keras_masking(feat, mv)
        h = O.dense(x, p["node_emb"], p["node_emb_bias"])
    else:
        h = M.neg1_masked_embedding(feat, p["node_emb"])
        mask = O.node_mask_from_features(feat)
    if kind:
        cfg = {"model_width": c["Dh"], f"sel_{kind}_features": sel, f"transform_{kind}": c["pe"][3]}
        op = {f"{kind}_emb.kernel": p["pe_kernel"], f"{kind}_emb.bias": p["pe_bias"]}
        h = h + (M.svd_embedding(pe, op, cfg, sg) if kind == "svd" else M.eig_embedding(pe, op, cfg, sg))
    if c["nv"]:
        h = torch.cat([p["virtual_node_emb"][None].expand(h.shape[0], -1, -1), h], dim=1)
        mask = torch.cat([torch.ones(h.shape[0], c["nv"], dtype=torch.bool), mask.bool()], dim=1)
    out = (h.detach(), mask.bool(), grads(h, p, c["d_h"]), grads(h, p, c["d_h_pos"]))
    _CACHE[key] = out
    return out


# ----------------------------------------------------------------------------------------------------- models -----
# one small instance of each model class with a positional encoding where its schemes have one
MODEL_RUNS = {
    "zinc": dict(use_svd=True, num_svd_features=16, sel_svd_features=8, transform_svd=True, random_neg=True, num_virtual_nodes=1),
    "pattern": dict(use_eig=True, num_eig_features=20, sel_eig_features=2, random_neg=True),
    "cluster": dict(use_eig=True, num_eig_features=20, sel_eig_features=20, random_neg=True),
    "cifar10": dict(use_svd=True, num_svd_features=16, sel_svd_features=8, transform_svd=True, random_neg=True, num_virtual_nodes=1),
    "mnist": dict(),
}


def model_run(which, gpu, lib=None):
    """One training-mode loss + backward of a small model on a seeded synthetic batch -> dict(loss, grads {keras name:
    tensor}, kernels (the library's launch names, when `lib` is given), grad_fn of h's producer).  The same seeds give the
    same parameters, batch and sign stream in every process."""
    import ctypes as C
    from egt_amd import model as M
    from egt_amd import training as T
    kw = MODEL_RUNS[which]
    cls, synth = dict(zinc=(M.ZincDCTransformer, T.SyntheticZinc), pattern=(M.PatternDCTransformer, T.SyntheticPattern),
                      cluster=(M.ClusterDCTransformer, T.SyntheticCluster), cifar10=(M.Cifar10DCTransformer, T.SyntheticCifar10),
                      mnist=(M.MnistDCTransformer, T.SyntheticMnist))[which]
    torch.manual_seed(7)
    model = cls(model_width=64, edge_width=64 if which == "zinc" else 8, model_height=1, upto_hop=4, random_mask_prob=0.0,
                **kw).to(gpu).train()
    data = synth(4, 4, nodes=(9, 21), seed=3)
    if kw.get("use_svd") or kw.get("use_eig"):
        data = T.WithPositional(data, "svd" if kw.get("use_svd") else "eig", 16 if kw.get("use_svd") else 20)
    b = {k: v.to(gpu) for k, v in next(iter(data)).items()}
    pe = {k: b[k] for k in ("singular_vectors", "eigen_vectors") if k in b}
    torch.manual_seed(11)                                   # the sign draw
    if lib is not None:
        lib.egt_prof_enable(2)
    try:
        if which in ("pattern", "cluster"):
            w = M.class_weights_from_sizes([3.0, 1.0] if which == "pattern" else [1.0] * 6, device=gpu)
            loss = model.classification_loss(b["node_features"], b["graph_matrix"], b["target"], w, **pe)[0]
        else:
            loss = model.graph_loss(b["node_features"], b["feature_matrix"], b["graph_matrix"], b["target"], **pe)[0]
        loss.backward()
        torch.cuda.synchronize()
        names = ""
        if lib is not None:
            buf = C.create_string_buffer(1 << 16)
            lib.egt_prof_names(buf, len(buf))
            names = buf.value.decode()
    finally:
        if lib is not None:
            lib.egt_prof_enable(0)
    grads = {k: p.grad.detach().cpu() for k, p in model.keras_named_parameters().items() if p.grad is not None}
    return dict(loss=loss.detach().cpu(), grads=grads, kernels=names, model=model, batch=b, pe=pe)
