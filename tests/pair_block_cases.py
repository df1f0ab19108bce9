"""Shapes and the host restatement of the launch plan of the large-head block operator (egt_pair_block_fwd / egt_pair_block_bwd,
egt_amd/csrc/egt_pair_node.hip).  No test functions here: tests/test_pair_block_cpu.py checks the table and the plan, the GPU
files run the rows.

Rows are (B, N, nodes): R = B N node rows scale through B so that e [B,N,N,32] stays tiny."""
from __future__ import annotations

import re

import torch

DH, DE, H = 512, 32, 8
TILE, K_STEP, MIN_CHUNK, MAX_CHUNKS, LN_ROWS = 128, 32, 256, 8, 64


def _seeded(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return [int(n) for n in torch.randint(1, N + 1, (B,), generator=g)]


TABLE = [
    (1, 8, [5]),                           # R below any tile
    (1, 37, [29]),                         # ragged
    (3, 24, [24, 0, 7]),                   # a graph with no node
    (5, 32, [32, 17, 1, 32, 20]),          # R = 160: two row tiles, the second ragged; one short chunk
    (2, 100, [100, 63]),
    (64, 16, _seeded(64, 16, 1)),          # R = 1024: several full row tiles, four full weight-gradient chunks
    (40, 27, _seeded(40, 27, 2)),          # R = 1080: ragged at every level (9 tiles, 5 chunks, 17 LN partials)
    (16, 16, _seeded(16, 16, 3)),          # R = 256: exactly one full chunk, full tiles
    (66, 32, _seeded(66, 32, 4)),          # R = 2112 > 8 * 256: chunks grow past the minimum (288 rows), the last one ragged
]
IDS = [f"b{B}_n{N}" for B, N, _ in TABLE]


def plan(R):
    """the library's plan_pn restated: dict(tiles, tile_ragged, rpc, chunks, chunk_ragged, ln_parts, reduce)"""
    per8 = -(-(-(-R // MAX_CHUNKS)) // K_STEP) * K_STEP          # ceil(ceil(R / 8) / 32) * 32
    rpc = max(MIN_CHUNK, per8)
    return dict(tiles=-(-R // TILE), tile_ragged=R % TILE != 0, rpc=rpc, chunks=-(-R // rpc), chunk_ragged=R % rpc != 0,
                ln_parts=-(-R // LN_ROWS), reduce=1)


def form(R):
    p = plan(R)
    return (f"tile={TILE}r/{p['tiles']}t{'/ragged' if p['tile_ragged'] else ''} wgrad={p['rpc']}r/{p['chunks']}c"
            f"{'/ragged' if p['chunk_ragged'] else ''} ln={LN_ROWS}r/{p['ln_parts']}p reduce={p['reduce']}")


_FORM = re.compile(r"^tile=(\d+)r/(\d+)t(/ragged)? wgrad=(\d+)r/(\d+)c(/ragged)? ln=(\d+)r/(\d+)p reduce=(\d+)$")


def parse(text):
    m = _FORM.match(text)
    assert m, text
    g = m.groups()
    return dict(tile=int(g[0]), tiles=int(g[1]), tile_ragged=g[2] is not None, rpc=int(g[3]), chunks=int(g[4]),
                chunk_ragged=g[5] is not None, ln_rows=int(g[6]), ln_parts=int(g[7]), reduce=int(g[8]))


def classes(p):
    """the classes of the launch plane a plan belongs to"""
    return {"one_tile" if p["tiles"] == 1 else "several_tiles", "ragged_tile" if p["tile_ragged"] else "full_tiles",
            "one_chunk" if p["chunks"] == 1 else "several_chunks", "ragged_chunk" if p["chunk_ragged"] else "full_chunks",
            "min_chunk" if p["rpc"] == MIN_CHUNK else "grown_chunk"}


ALL_CLASSES = {"one_tile", "several_tiles", "ragged_tile", "full_tiles", "one_chunk", "several_chunks", "ragged_chunk", "full_chunks",
               "min_chunk", "grown_chunk"}


def desc(B, N, training=False, p=0.0, seed=0, clip=True, flags=None):
    from egt_amd import _lib as L
    f = L.BF_GATE | (L.BF_CLIP if clip else 0) | (L.BF_TRAINING if training else 0)
    return L.BlockDesc(B=B, N=N, H=H, d=DH // H, De=DE, dtype=L.EGT_F32, flags=f if flags is None else flags,
                       clip_lo=-5.0 if clip else 0.0, clip_hi=5.0 if clip else 0.0, random_mask_prob=p, ln_eps=1e-3, reserved=0,
                       seed=seed, seed_device=None)


def make(B, N, nodes, seed=None, scale=1.0):
    """(inp, params): the inputs of tests/test_pair_gpu.py's cases, h times `scale`"""
    from oracle import egt_oracle as O
    g = torch.Generator().manual_seed(1000 + B * 131 + N if seed is None else seed)
    params = O.init_block_params(DH, DE, H, generator=g, randomize_norm=True)
    h = torch.randn(B, N, DH, generator=g) * scale
    e = torch.randn(B, N, N, DE, generator=g) * 1.2 + 0.2
    dh = torch.randn(B, N, DH, generator=g)
    de = torch.randn(B, N, N, DE, generator=g)
    mask = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate(nodes):
        mask[b, :n] = True
    return dict(h=h, e=e, mask=mask, attn_mask=None, rand_mask=None, dh=dh, de=de), params


ATTRS = dict(num_heads=H, gate_attention=True, edge_activation=None, edge_channel_type="residual")
_ORACLES = {}


def oracle(i, dtype=torch.float64):
    """the fp64 (or fp32) oracle of table row i, computed once per process and shared"""
    import cases as CS
    key = (i, dtype)
    if key not in _ORACLES:
        inp, params = make(*TABLE[i])
        _ORACLES[key] = CS.block_oracle(inp, params, ATTRS, dtype=dtype)
    return _ORACLES[key]
