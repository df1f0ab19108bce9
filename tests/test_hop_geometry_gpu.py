"""k_hop_chain, k_hop_step and k_dist_target across their launch plane (tests/hop_geometry.py: the workgroup shape follows B and
N together) against the fp64 references: the hop planes of 0/1 adjacencies bit for bit against MO.stack_hops, the weighted
unclipped planes within the tolerance of tests/test_model.py, the distance target bit for bit against distance_ref.ref_target,
and -- from the C ABI's launch profiler -- the kernels the shape was chosen to run.  The per-hop kernels at shapes that would
chain run in a child process, where EGT_NO_HOP_CHAIN is set before the library reads it."""
import os
import subprocess
import sys

import pytest
import torch

import distance_ref as DR
import hop_geometry as HG

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
_id = lambda r: f"{r[0]}x{r[1]}"


@pytest.mark.parametrize("row", list(HG.EMBED_ROWS), ids=_id)
def test_hop_planes_vs_oracle(row, gpu, egt_lib):
    p = HG.check_hop_planes(*row, gpu, egt_lib)
    assert p["kind"] == HG.EMBED_ROWS[row]["kind"]


@pytest.mark.parametrize("row", HG.DIST_ROWS, ids=_id)
def test_distance_target_vs_reference(row, gpu, egt_lib):
    HG.check_distance_target(*row, gpu, egt_lib)


def test_distance_target_at_the_uint8_ceiling(gpu, egt_lib):
    from egt_amd import distance_target
    adj = DR.make_graphs(19)
    ref = DR.ref_target(adj, 255)
    assert int(ref.max()) == 255
    assert torch.equal(distance_target(adj.to(gpu), 255).cpu().long(), ref)


def test_distance_target_refuses_what_does_not_fit(gpu, egt_lib):
    from egt_amd import distance_target, _lib as L
    B, N = 2, 193
    assert HG.plan(B, N, HG.T_DIST, dist=True)["kind"] == "refused"
    adj = HG.graphs(B, N)[0].to(gpu)
    out = torch.full((B, N, N), 7, dtype=torch.uint8, device=gpu)
    assert egt_lib.egt_distance_target(L.ptr(adj), B, N, HG.T_DIST, L.ptr(out), L.current_stream()) == L.EGT_E_SHAPE
    assert b"N <= 192" in egt_lib.egt_last_error_string()
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7, "a refused call writes nothing"
    with pytest.raises(AssertionError, match="distance target"):
        distance_target(adj, HG.T_DIST)


def test_per_hop_kernels_without_the_chain(gpu, egt_lib):
    """EGT_NO_HOP_CHAIN (README: a switch for tests): k_hop_first + k_hop_step at HG.NOCHAIN_ROWS, the same comparisons and the
    launch counts, in a fresh interpreter"""
    env = dict(os.environ, EGT_NO_HOP_CHAIN="1")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "hop_geometry.py"), "--no-chain"], cwd=os.path.dirname(TESTS), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "no-chain ok" in r.stdout and r.stdout.count("k_hop_step") == len(HG.NOCHAIN_ROWS), r.stdout
