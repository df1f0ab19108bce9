"""The shape table of tests/hop_geometry.py reaches the launch plane it claims to, on inputs that can tell a wrong kernel from a
right one (no GPU): plan() -- the restated host rule of embed_planes / egt_distance_target -- gives every row the class it is
annotated with, the classes cover the plane, the sparse graphs are not degenerate on the fp64 reference, and the weighted
comparison is fair (MO.stack_hops in fp32 on the CPU stays within CAP of the tolerance the GPU test applies)."""
import pytest
import torch

import distance_ref as DR
import hop_geometry as HG
from util import margin

CAP = 0.25          # as tests/conditioning.py: a kernel that fails is at least four times worse than plain fp32


@pytest.fixture(autouse=True)
def _one_thread(monkeypatch):
    monkeypatch.delenv("EGT_NO_HOP_CHAIN", raising=False)     # plan() follows the switch, as the library does
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("row", list(HG.EMBED_ROWS), ids=lambda r: f"{r[0]}x{r[1]}")
def test_embed_rows_have_their_class(row):
    p = HG.plan(*row, HG.K_HOPS)
    for k, v in HG.EMBED_ROWS[row].items():
        assert p[k] == v, (row, k, p)
    if p["kind"] == "chain":
        assert p["tiles"] <= HG.NW * HG.MAXT and p["lds"] <= HG.LDS_CAP and p["NB"] * p["CT"] >= p["RT"]
    if row not in HG.DIST_ONLY_ROWS:                      # the distance target takes the same shape there
        assert HG.plan(*row, HG.T_DIST, dist=True) == p


@pytest.mark.parametrize("row", list(HG.DIST_ONLY_ROWS), ids=lambda r: f"{r[0]}x{r[1]}")
def test_distance_rows_have_their_class(row):
    p = HG.plan(*row, HG.T_DIST, dist=True)
    for k, v in HG.DIST_ONLY_ROWS[row].items():
        assert p[k] == v, (row, k, p)


def test_the_table_covers_the_launch_plane():
    ps = [HG.plan(B, N, HG.K_HOPS) for B, N in HG.EMBED_ROWS]
    chain = [p for p in ps if p["kind"] == "chain"]
    cts = {p["CT"] for p in chain}
    assert {2, 3} <= cts and any(c >= 5 for c in cts)
    assert any(p["rem"] for p in chain) and any(p["per_wave"] == HG.MAXT for p in chain)
    assert any(p["CT"] == p["RT"] for p in chain) and any(p["kind"] == "step" for p in ps)
    assert {"lds", "tiles"} <= {p["cut"] for p in chain}
    # CT = 1 chained: the shapes of tests/test_model.py (B <= 3) and, for the distance target, its hp = 0 rows
    ds = [HG.plan(B, N, HG.T_DIST, dist=True) for B, N in HG.DIST_ROWS]
    assert all(p["kind"] == "chain" for p in ds)
    assert any(p["CT"] == 1 for p in ds) and any(p["hp"] == 0 for p in ds)
    assert {p["CT"] for p in ds} >= cts
    # the boundaries themselves
    assert HG.plan(47, 176, 4)["kind"] == "chain" and HG.plan(1, 177, 4)["kind"] == "step"
    assert HG.plan(1, 176, 5, dist=True)["hp"] == 4 and HG.plan(1, 177, 5, dist=True)["hp"] == 0
    assert HG.plan(1, 192, 5, dist=True)["kind"] == "chain" and HG.plan(1, 193, 5, dist=True)["kind"] == "refused"
    assert HG.plan(64, 150, 1)["kind"] == "step", "upto_hop = 1: plane 0 alone"


def test_no_chain_rows_reach_the_edges_of_k_hop_step():
    rows = HG.NOCHAIN_ROWS
    assert all(HG.plan(B, N, HG.K_HOPS)["kind"] == "chain" for B, N in rows), "they chain unless the switch is set"
    assert all(B > 1 for B, _ in rows)
    assert {N % 4 for _, N in rows} == {0, 1, 2, 3}
    assert {(N + 31) // 32 for _, N in rows} == {1, 2, 3}
    assert any(N < 16 for _, N in rows) and any(N % 32 == 0 for _, N in rows)


ALL_ROWS = sorted(set(HG.EMBED_ROWS) | set(HG.DIST_ROWS) | set(HG.NOCHAIN_ROWS))


@pytest.mark.parametrize("row", ALL_ROWS, ids=lambda r: f"{r[0]}x{r[1]}")
def test_graphs_are_not_degenerate(row):
    """on the fp64 reference alone: a share of ones inside (0.005, 0.9) in every compared plane, both values in every 16-column
    block of the last plane of an unpadded graph, every distance class 0..T; the recipe's padded and empty graphs are there"""
    from oracle import egt_model_oracle as MO
    B, N = row
    adj, n_last = HG.graphs(B, N)
    assert torch.equal(adj, adj.transpose(1, 2)) and set(adj.unique().tolist()) == {0.0, 1.0}
    assert N // 2 <= n_last < N and float(adj[B - 1, n_last:].abs().max()) == 0.0 and float(adj[B - 1, :n_last].max()) == 1.0
    if B >= 3:
        assert float(adj[1].abs().max()) == 0.0
    if row in HG.EMBED_ROWS or row in HG.NOCHAIN_ROWS:
        hops = MO.stack_hops(adj.double(), HG.K_HOPS)
        shares = [float(hops[..., k].mean()) for k in range(HG.K_HOPS)]
        print(f"B={B} N={N}: shares of ones per plane {['%.4f' % s for s in shares]}")
        assert all(0.005 < s < 0.9 for s in shares), shares
        for b in HG.unpadded(B):
            last = hops[b, :, :, -1]
            for c in range(0, N, 16):
                blk = last[:, c:c + 16]
                assert 0.0 < float(blk.mean()) < 1.0, f"graph {b}, columns {c}..: one value only"
    if row in HG.DIST_ROWS:
        t = DR.ref_target(adj, HG.T_DIST)
        assert sorted(t.unique().tolist()) == list(range(HG.T_DIST + 1)), "every class 0..T occurs"


@pytest.mark.parametrize("row", sorted(set(HG.EMBED_ROWS) | set(HG.NOCHAIN_ROWS)), ids=lambda r: f"{r[0]}x{r[1]}")
def test_weighted_comparison_is_fair(row):
    """the unclipped planes of the weighted adjacency: MO.stack_hops in fp32 on the CPU against itself in fp64, under the tolerance
    of the GPU test (measured: 0.001 - 0.002 of it at the table's shapes)"""
    from oracle import egt_model_oracle as MO
    adjw = HG.weights(*row)
    assert float(adjw.max()) < 1.0 and int((adjw > 0).sum()) == int(HG.graphs(*row)[0].sum())
    ref = MO.stack_hops(adjw.double(), HG.K_HOPS, clip_hops=False)
    f32 = MO.stack_hops(adjw, HG.K_HOPS, clip_hops=False)
    worst = margin(f32, ref, **HG.WEIGHTED_TOL)
    print(f"B={row[0]} N={row[1]}: fp32 stack_hops reaches {worst:.4f} of the tolerance")
    assert worst <= CAP, f"{row}: the fp32 reference reaches {worst:.3f} of the tolerance (cap {CAP})"


def test_uint8_ceiling_case():
    """T = 255 at the N = 19 graphs of tests/distance_ref.py: the lollipop's triangle makes walks of every length, so pairs reach
    the top of the uint8 range, and the edgeless graph stays 0"""
    t = DR.ref_target(DR.make_graphs(19), 255)
    assert int(t.max()) == 255 and int(t[2].max()) == 0 and len(t.unique()) > 8
