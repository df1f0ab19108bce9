"""The launch plane of the two kernels that walk the hop chain with a graph's adjacency in LDS -- TEST INFRASTRUCTURE shared by
tests/test_hop_geometry_cpu.py and tests/test_hop_geometry_gpu.py (no test functions here).

plan() restates the host rule of

    embed_planes          egt_amd/csrc/egt_embed.hip   (k_hop_chain, else k_hop_first + one k_hop_step per hop)
    egt_distance_target   egt_amd/csrc/egt_head.hip    (k_dist_target)

which pick the workgroup shape from B and N TOGETHER: ct = RT * B / 256 column tiles per workgroup (RT = ceil(N / 16) row
tiles), cut back until RT * ct <= 64 tile pairs (8 waves x HOP_MAXT = 8 pairs) and the LDS image -- the zero-padded adjacency
[R16][R16 + 4] plus the column block [R16][16 ct + hp] of the current plane, fp32 -- is at most 160 KiB; NB = ceil(RT / ct)
workgroups per graph.  Where one column tile does not fit, the embedding falls back to a launch per hop and the distance target
drops the plane's row padding (hp = 0; N in 177..192) or refuses the shape (N > 192).

Run as a script (`python tests/hop_geometry.py --no-chain`) it is the child process of test_hop_geometry_gpu.py: the library reads
EGT_NO_HOP_CHAIN once per process, so the per-hop kernels at shapes that would chain need an interpreter of their own.
"""
import functools
import os
import sys

import torch

NW, MAXT = 8, 8                 # HOP_NW / DT_NW, HOP_MAXT / DT_MAXT
LDS_CAP = 160 * 1024
DT_MAX_N = 192
K_HOPS = 4                      # upto_hop of the embedding runs
T_DIST = 5                      # classes 0..5 of the distance target runs
WEIGHTED_TOL = dict(rtol=1e-4, arel=1e-5)   # the weighted planes' tolerance of tests/test_model.py::test_edge_embed_vs_oracle


def lds_bytes(N, ct, hp=4):
    R16 = (N + 15) // 16 * 16
    return (R16 * (R16 + 4) + R16 * (16 * ct + hp)) * 4


def plan(B, N, K, dist=False):
    """dict(kind, RT, CT, NB, tiles, per_wave, rem, hp, lds, cut): kind 'chain' (k_hop_chain / k_dist_target), 'step' (per-hop
    launches; the embedding only) or 'refused' (the distance target only).  tiles = RT * CT pairs per workgroup, per_wave the most
    one wave owns, rem = RT % CT (!= 0: the last workgroup of a graph owns column tiles beyond R16), cut: what shrank ct
    ('' | 'tiles' | 'lds' | 'tiles+lds')."""
    RT = (N + 15) // 16
    ct = min(max(RT * B // 256, 1), RT)
    hp, cut = 4, []
    if dist:
        if N > DT_MAX_N:
            return dict(kind="refused", RT=RT, CT=0, NB=0, tiles=0, per_wave=0, rem=0, hp=hp, lds=0, cut="")
        while ct > 1 and (RT * ct > NW * MAXT or lds_bytes(N, ct, hp) > LDS_CAP):
            cut.append("tiles" if RT * ct > NW * MAXT else "lds")
            ct -= 1
        if lds_bytes(N, ct, hp) > LDS_CAP:
            hp = 0
        fits = RT * ct <= NW * MAXT and lds_bytes(N, ct, hp) <= LDS_CAP
        kind = "chain" if fits else "refused"
    else:
        while ct > 1 and RT * ct > NW * MAXT:
            cut.append("tiles"); ct -= 1
        while ct > 1 and lds_bytes(N, ct) > LDS_CAP:
            cut.append("lds"); ct -= 1
        fits = K > 1 and RT * ct <= NW * MAXT and lds_bytes(N, ct) <= LDS_CAP
        kind = "chain" if fits and not os.environ.get("EGT_NO_HOP_CHAIN") else "step"
    if kind != "chain":
        return dict(kind=kind, RT=RT, CT=0, NB=0, tiles=0, per_wave=0, rem=0, hp=hp, lds=0, cut="")
    tiles = RT * ct
    return dict(kind=kind, RT=RT, CT=ct, NB=(RT + ct - 1) // ct, tiles=tiles, per_wave=(tiles + NW - 1) // NW, rem=RT % ct, hp=hp,
                lds=lds_bytes(N, ct, hp), cut="+".join(sorted(set(cut))))


# (B, N): the class the row is there for, as plan() fields that must hold -- for the embedding (K = 4) and, under "dist", for the
# distance target where it differs.  test_hop_geometry_cpu.py checks every annotation against plan().
EMBED_ROWS = {
    (192, 50): dict(kind="chain", CT=3, NB=2, rem=1),                       # CT = 3, a remainder block
    (256, 37): dict(kind="chain", CT=3, RT=3, NB=1),                        # CT = RT: one workgroup per graph
    (256, 128): dict(kind="chain", CT=8, tiles=64, per_wave=8, NB=1),       # HOP_MAXT full
    (128, 150): dict(kind="chain", CT=5, NB=2, per_wave=7, rem=0),          # the CIFAR10 training shape
    (90, 150): dict(kind="chain", CT=3, NB=4, rem=1),
    (47, 176): dict(kind="chain", CT=2, NB=6, rem=1),                       # the largest N that chains
    (3, 177): dict(kind="step"),                                            # smallest N on k_hop_step, B > 1, N odd
    # the two loops that cut ct back, which none of the rows above enters
    (94, 176): dict(kind="chain", CT=3, NB=4, rem=2, cut="lds"),            # ct = 4 does not fit: 163328 of 163840 bytes at 3
    (256, 144): dict(kind="chain", CT=7, NB=2, rem=2, per_wave=8, cut="tiles"),   # ct = 9, 8 are more than 64 pairs
}
DIST_ONLY_ROWS = {
    (3, 177): dict(kind="chain", CT=1, hp=0),                               # the hp = 0 branch
    (3, 192): dict(kind="chain", CT=1, hp=0, RT=12),                        # DT_MAX_N
    (2, 193): dict(kind="refused"),                                         # must return EGT_E_SHAPE
}
DIST_ROWS = [r for r in EMBED_ROWS if r != (3, 177)] + [(3, 177), (3, 192)]

# the per-hop kernels under EGT_NO_HOP_CHAIN: k_hop_step's own edges -- T2 = ceil(N / 32) blocks a side (1, 2, 3), b > 0,
# float4 loads only where jb + 3 < N (N % 4 = 1, 2, 3, 0), N below one MFMA tile
NOCHAIN_ROWS = [(3, 5), (2, 31), (3, 33), (2, 64), (2, 70)]


@functools.lru_cache(maxsize=None)
def graphs(B, N):
    """[B,N,N] fp32, never modified: symmetric 0/1 adjacencies, A = D or D^T of a matrix D whose elements (the diagonal too) are 1
    with probability 1.25 / N (as tests/test_model.py draws its graphs: about 2.5 neighbours per node); the LAST graph padded (n real nodes, n drawn from [N/2, N), zero rows and columns behind them); from B = 3 on graph 1
    has no edges at all (at B = 2 graph 0 must stay the unpadded graph with edges).  Returns (adj, n_last)."""
    g = torch.Generator().manual_seed(7919 * B + N)
    adj = (torch.rand(B, N, N, generator=g) < 1.25 / N).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float()
    n_last = int(torch.randint(N // 2, N, (1,), generator=g)) if N > 1 else N
    adj[B - 1, n_last:, :] = 0.0
    adj[B - 1, :, n_last:] = 0.0
    if B >= 3:
        adj[1] = 0.0
    return adj, n_last


@functools.lru_cache(maxsize=None)
def weights(B, N):
    """uniform (0, 1) edge weights for the unclipped, weighted planes"""
    g = torch.Generator().manual_seed(104729 * B + N)
    return graphs(B, N)[0] * torch.rand(B, N, N, generator=g)


def unpadded(B):
    """the graphs of a batch that are neither padded nor empty"""
    return [b for b in range(B - 1) if not (B >= 3 and b == 1)]


# ----------------------------------------------------------------------------------------------- GPU comparisons -----
def launch_counts(lib, fn):
    """run fn() under the C ABI's launch profiler: {kernel name: launches}"""
    import ctypes as C
    lib.egt_prof_filter(b""); lib.egt_prof_enable(2)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.egt_prof_enable(0)
    buf = C.create_string_buffer(4096)
    lib.egt_prof_names(buf, 4096)
    count = {}
    for name in buf.value.decode().split():
        cnt, ms = C.c_int64(0), C.c_double(0.0)
        lib.egt_prof_read(name.encode(), C.byref(cnt), C.byref(ms))
        if cnt.value:
            count[name] = cnt.value
    return out, count


def check_hop_planes(B, N, gpu, lib, K=K_HOPS):
    """edge_embed(..., return_hops=True) at De = 4 with a one-row table: the planes of the 0/1 adjacency bit for bit against
    MO.stack_hops in fp64, the weighted unclipped planes within WEIGHTED_TOL, and which kernels ran against plan()"""
    from egt_amd import edge_embed
    from oracle import egt_model_oracle as MO
    from util import assert_close
    adj, _ = graphs(B, N)
    p = plan(B, N, K)
    fm = torch.full((B, N, N), -1, dtype=torch.int32, device=gpu)
    g = torch.Generator().manual_seed(N)
    table, W, b = torch.zeros(1, 4, device=gpu), (torch.randn(K, 4, generator=g) * 0.3).to(gpu), torch.zeros(4, device=gpu)
    (_, hops), count = launch_counts(lib, lambda: edge_embed(fm, adj.to(gpu), table, W, b, return_hops=True))
    if p["kind"] == "chain":
        assert count.get("k_hop_chain") == 1 and "k_hop_step" not in count and "k_hop_first" not in count, (p, count)
    else:
        assert count.get("k_hop_first") == 1 and count.get("k_hop_step", 0) == K - 1 and "k_hop_chain" not in count, (p, count)
    ref = MO.stack_hops(adj.double(), K)
    got = hops.permute(1, 2, 3, 0).cpu()
    if not torch.equal(got, ref.float()):
        bad = (got != ref.float()).nonzero()
        raise AssertionError(f"hop planes of a 0/1 adjacency are exact: {len(bad)} elements differ at B={B} N={N} ({p}); first "
                             f"(b, l, m, k) = {bad[0].tolist()}; graphs {sorted(set(bad[:, 0].tolist()))[:8]}, column tiles "
                             f"{sorted(set((bad[:, 2] // 16).tolist()))}, planes {sorted(set(bad[:, 3].tolist()))}")
    adjw = weights(B, N)
    _, hw = edge_embed(fm, adjw.to(gpu), table, W, b, clip_hops=False, return_hops=True)
    assert_close(hw.permute(1, 2, 3, 0), MO.stack_hops(adjw.double(), K, clip_hops=False), name=f"weighted hops B={B} N={N}",
                 **WEIGHTED_TOL)
    return p


def check_distance_target(B, N, gpu, lib, T=T_DIST):
    import distance_ref as DR
    from egt_amd import distance_target
    adj, _ = graphs(B, N)
    got, count = launch_counts(lib, lambda: distance_target(adj.to(gpu), T))
    assert count == {"k_dist_target": 1}, count
    ref = DR.ref_target(adj, T)
    assert got.dtype == torch.uint8
    if not torch.equal(got.cpu().long(), ref):
        bad = (got.cpu().long() != ref).nonzero()
        raise AssertionError(f"distance target B={B} N={N} T={T} ({plan(B, N, T, dist=True)}): {len(bad)} elements differ; first "
                             f"(b, l, m) = {bad[0].tolist()}; column tiles {sorted(set((bad[:, 2] // 16).tolist()))}")


def _no_chain_child():
    """the per-hop kernels at shapes that would chain; exit status 0 and the line 'no-chain ok' when every comparison held"""
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert os.environ.get("EGT_NO_HOP_CHAIN"), "run with EGT_NO_HOP_CHAIN=1"
    from egt_amd import _lib
    lib, gpu = _lib.load(), torch.device("cuda:0")
    for B, N in NOCHAIN_ROWS:
        p = check_hop_planes(B, N, gpu, lib)
        assert p["kind"] == "step"
        print(f"B={B} N={N}: k_hop_first + {K_HOPS - 1} x k_hop_step", flush=True)
    print("no-chain ok", flush=True)


if __name__ == "__main__":
    if sys.argv[1:] != ["--no-chain"]:
        sys.exit("usage: EGT_NO_HOP_CHAIN=1 python tests/hop_geometry.py --no-chain")
    _no_chain_child()
