"""FlatOptimizer on the GPU against torch.optim in fp64 (optim_ref.py: the sets, the recipes, the parity rule), and the
properties the kernel promises: position independence, determinism, capture, zero_grad, stale pointers, checkpoint
interchange, the training driver.  EGT_FLAT_OPTIM_MARGINS=<file> additionally writes the worst measured ratio per
(algorithm, recipe) to that file (profiles/flat_optim_margins.json is such a dump)."""
import json
import os

import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_margins():
    yield
    path = os.environ.get("EGT_FLAT_OPTIM_MARGINS")
    if path and MARGINS:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(tolerance="per tensor 4 E + 2 ulp(max |oracle|), E = torch's fp32 optimizer against the fp64 oracle on the "
                                     "same case; ratio = worst |error| / tolerance (<= 1 passes)",
                           worst_ratio={a: {r: dict(ratio=round(v[0], 4), where=v[1]) for r, v in sorted(d.items())}
                                        for a, d in sorted(MARGINS.items())}), f, indent=1, sort_keys=True)


def _hold(algo, recipe, where, got, own, ref):
    """(p, m, v) triples of lists under the parity rule; records and returns the worst ratio"""
    worst = (0.0, "")
    for what, a, b, c in zip(("p", "m", "v"), got, own, ref):
        if c is None:
            continue
        r, i = R.worst_ratio(a, b, c, what)
        print(f"{algo}/{recipe}/{where}: {what} ratio {r:.4f} (tensor {i})")
        if r > worst[0]:
            worst = (r, f"{where}:{what}[{i}]")
    slot = MARGINS.setdefault(algo, {})
    if worst[0] >= slot.get(recipe, (-1.0, ""))[0]:
        slot[recipe] = worst
    assert worst[0] <= 1.0, f"{algo}/{recipe}/{where}: {worst[1]} is at {worst[0]:.3f} of 4 E + 2 ulp"
    return worst[0]


CASES = [(a, r, s, c) for a in R.ALGOS for r in R.RECIPES for s in R.SETS for c in (False, True)]


@pytest.mark.parametrize("algo,recipe,pset,clip", CASES, ids=[f"{a}-{r}-{s}-{'clip' if c else 'noclip'}" for a, r, s, c in CASES])
def test_parity_with_torch_optim_in_fp64(algo, recipe, pset, clip, gpu, egt_lib):
    p0, g = R.params0(pset), R.grads(pset, recipe)
    cv = R.CLIP if clip else None
    ref = R.oracle(algo, pset, recipe, clip)
    own = R.run_torch(algo, p0, g, torch.float32, device=gpu, clip=cv)[:3]
    got = R.run_flat(algo, p0, g, gpu, clip=cv)
    assert got[3].step_count() == R.K
    _hold(algo, recipe, f"{pset}{'-clip' if clip else ''}", got[:3], own, ref)


def _late_state(algo, pset, step=1000):
    """a torch.optim state_dict at `step`: moments as a long run leaves them (fp32 values)"""
    g = R._gen("late", algo, pset)
    mk, vk = R.MOMENTS[algo]
    state = {}
    for i, s in enumerate(R.shapes(pset)):
        d = {"step": torch.tensor(float(step))}
        if mk:
            d[mk] = torch.randn(*s, generator=g) * 0.1
        d[vk] = torch.rand(*s, generator=g) * 0.5 + 1e-4
        state[i] = d
    groups = R.torch_optimizer(algo, [torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"]
    groups[0]["params"] = list(range(len(state)))
    return {"state": state, "param_groups": groups}


@pytest.mark.parametrize("algo", ["adam", "rmsprop"])
def test_late_step_bias_corrections(algo, gpu, egt_lib):
    """t = 1001..1003: 1 - 0.999^t is 0.63; with steps 1..5 of the parity test this holds the corrections at both ends"""
    import copy
    pset = "ragged"
    p0, g = R.params0(pset), R.grads(pset, "normal")[:3]
    sd = _late_state(algo, pset)
    ref = R.run_torch(algo, p0, g, torch.float64, state=copy.deepcopy(sd))[:3]
    own = R.run_torch(algo, p0, g, torch.float32, device=gpu, state=copy.deepcopy(sd))[:3]
    got = R.run_flat(algo, p0, g, gpu, state=copy.deepcopy(sd))
    assert got[3].step_count() == 1003
    _hold(algo, "late_step", pset, got[:3], own, ref)


def _same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: parameter {i} differs"


@pytest.mark.parametrize("algo", R.ALGOS)
def test_position_independence(algo, gpu, egt_lib):
    for pset in R.SETS:
        p0, g = R.params0(pset), R.grads(pset, "mixed_sign_outliers")
        a = R.run_flat(algo, p0, g, gpu, clip=R.CLIP)
        b = R.run_flat(algo, p0, g, gpu, clip=R.CLIP, order=list(range(len(p0)))[::-1])
        for k, what in enumerate(("p", "m", "v")):
            if a[k] is not None:
                _same_bits(a[k], b[k], f"{pset} reversed {what}")
    # every parameter of `ragged` at an odd float offset of one carrier tensor; the floats around them stay as they were
    p0, g = R.params0("ragged"), R.grads("ragged", "normal")
    offs, off = [], 1
    for p in p0:
        off += (1 - off % 2) + 2                       # odd, at least two floats after the previous parameter
        offs.append(off)
        off += p.numel()
    assert all(o % 2 == 1 for o in offs) and {o % 4 for o in offs} == {1, 3}
    a = R.run_flat(algo, p0, g, gpu)
    c = R.run_flat(algo, p0, g, gpu, carrier_offsets=offs)
    for k, what in enumerate(("p", "m", "v")):
        if a[k] is not None:
            _same_bits(a[k], c[k], f"carrier {what}")
    carrier, ranges = c[4]
    keep = torch.ones(carrier.numel(), dtype=torch.bool, device=gpu)
    for lo, hi in ranges:
        keep[lo:hi] = False
    assert bool((carrier[keep] == 123.0).all()), "a float outside the parameters was written"


@pytest.mark.parametrize("algo", R.ALGOS)
def test_two_runs_are_bitwise_equal_and_zero_grad_changes_nothing_else(algo, gpu, egt_lib):
    p0, g = R.params0("ragged"), R.grads("ragged", "normal")
    a, b = R.run_flat(algo, p0, g, gpu, clip=R.CLIP), R.run_flat(algo, p0, g, gpu, clip=R.CLIP)
    z = R.run_flat(algo, p0, g, gpu, clip=R.CLIP, zero_grad=True)
    for k, what in enumerate(("p", "m", "v")):
        if a[k] is not None:
            _same_bits(a[k], b[k], f"second run {what}")
            _same_bits(a[k], z[k], f"zero_grad {what}")
    assert float(z[3].flat_grads.flat.abs().max()) == 0.0 and float(a[3].flat_grads.flat.abs().max()) > 0.0


@pytest.mark.parametrize("algo", R.ALGOS)
def test_captured_step_replays_like_eager_steps(algo, gpu, egt_lib):
    from egt_amd.optim import FlatOptimizer
    p0, g = R.params0("ragged"), R.grads("ragged", "normal")[0]
    lrs = [1e-3, 5e-4, 2e-3]
    eager = R.run_flat(algo, p0, [g] * 3, gpu, lrs=lrs, lr=lrs[0])
    ps, flat = R.make_flat(p0, gpu)
    opt = FlatOptimizer(ps, flat, algo=algo, lr=lrs[0])
    for p, t in zip(ps, g):
        p.grad.copy_(t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for lr in lrs:
        opt.set_lr(lr)
        graph.replay()
    torch.cuda.synchronize()
    assert opt.step_count() == 3 and opt.param_groups[0]["lr"] == lrs[-1]
    _same_bits(eager[0], [p.detach() for p in ps], "graphed p")
    if eager[2] is not None:
        _same_bits(eager[2], R.split(opt._v, [tuple(p.shape) for p in ps]), "graphed v")


def test_a_moved_parameter_is_followed_and_the_old_storage_left_alone(gpu, egt_lib):
    from egt_amd.optim import FlatOptimizer
    p0, g = R.params0("ragged"), R.grads("ragged", "normal")
    want = R.run_flat("adam", p0, g[:2], gpu)[0]
    ps, flat = R.make_flat(p0, gpu)
    opt = FlatOptimizer(ps, flat, algo="adam", lr=R.LR)
    for k in range(2):
        for p, t in zip(ps, g[k]):
            p.grad.copy_(t)
        if k == 1:
            old = [ps[4].data, ps[0].data]
            snap = [t.clone() for t in old]
            ps[4].data = ps[4].data.clone()
            ps[0].data = ps[0].data.clone()
            assert not opt.pointers_current()
        opt.step()
        assert opt.pointers_current()
    _same_bits(want, [p.detach() for p in ps], "after the move")
    for t, s in zip(old, snap):
        assert torch.equal(t, s), "the old storage was written"
    ps[1].data = ps[1].data.double()
    with pytest.raises(ValueError, match="fp32"):
        opt.step()


@pytest.mark.parametrize("algo", R.ALGOS)
def test_checkpoint_interchange_with_torch_optim(algo, gpu, egt_lib):
    import copy
    pset = "ragged"
    p0, g6 = R.params0(pset), R.grads(pset, "normal", 6, 1)
    ref = R.run_torch(algo, p0, g6, torch.float64)[:3]
    own = R.run_torch(algo, p0, g6, torch.float32, device=gpu)[:3]
    # torch for 3 steps, then FlatOptimizer for 3
    t3 = R.run_torch(algo, p0, g6[:3], torch.float32, device=gpu)
    got = R.run_flat(algo, t3[0], g6[3:], gpu, state=copy.deepcopy(t3[3].state_dict()))
    assert got[3].step_count() == (3 if algo == "sgd" else 6)
    _hold(algo, "interchange", "torch->flat", got[:3], own, ref)
    # FlatOptimizer for 3 steps, then torch for 3
    f3 = R.run_flat(algo, p0, g6[:3], gpu)
    sd = f3[3].state_dict()
    fresh = R.torch_optimizer(algo, [torch.nn.Parameter(p.clone()) for p in f3[0]]).state_dict()
    assert set(sd["param_groups"][0]) == set(fresh["param_groups"][0]) and set(sd["state"]) == set(t3[3].state_dict()["state"])
    for i, d in sd["state"].items():
        assert set(d) == set(t3[3].state_dict()["state"][i]) and d["step"].dtype == torch.float32 and float(d["step"]) == 3.0
    back = R.run_torch(algo, f3[0], g6[3:], torch.float32, device=gpu, state=sd)[:3]
    _hold(algo, "interchange", "flat->torch", back, own, ref)
    if algo != "sgd":
        bad = copy.deepcopy(sd)
        bad["state"][1]["step"] = torch.tensor(9.0)
        with pytest.raises(ValueError, match="one counter"):
            f3[3].load_state_dict(bad)


# ---- the training driver -------------------------------------------------------------------------------------------
def _scheme(tmp_path, tag, fused, graph, T, gpu):
    torch.manual_seed(0)
    cfg = dict(scheme="zinc.svd", model_name=tag, model_width=32, edge_width=32, batch_size=8, num_epochs=1, initial_lr=2e-3,
               use_svd=False, model_height=2, upto_hop=4, random_mask_prob=0.0, gradient_clipval=0.02, use_hipgraph=graph,
               fused_optimizer=fused, save_path=str(tmp_path / tag))
    s = T.ZincSVDScheme(cfg, device=gpu, print_fn=lambda *a: None)
    s.load_model()
    return s


def _train(s, batches, record=None):
    """train_step over the batches; record: list that receives every step's (clipped) gradients as the optimizer sees them"""
    if record is not None:
        inner = s.optimizer.step

        def step(*a, **k):
            record.append(tuple(p.grad.detach().cpu().clone() for p in s.params))
            return inner(*a, **k)
        s.optimizer.step = step
    losses = [s.train_step(b) for b in batches]
    if record is not None:
        s.optimizer.step = inner
    return losses


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hipgraph"])
def test_driver_switch_on_against_off(graph, tmp_path, gpu, egt_lib):
    import egt_amd.training as T
    from egt_amd.optim import FlatOptimizer
    batches = list(T.SyntheticZinc(32, 8, seed=1, pad_multiple=1))[:4]
    off, on = _scheme(tmp_path, "off", False, graph, T, gpu), _scheme(tmp_path, "on", True, graph, T, gpu)
    assert isinstance(on.optimizer, FlatOptimizer) and isinstance(off.optimizer, torch.optim.Adam) and on.flat is not None
    assert on.optimizer.zero_grad_in_step == (not graph) and on.optimizer.clip_value == 0.02
    p0 = [p.detach().cpu().clone() for p in off.params]
    _same_bits(p0, [p.detach().cpu() for p in on.params], "initial parameters")
    rec = []
    l_off, l_on = _train(off, batches, rec), _train(on, batches)
    assert l_on[0] == l_off[0] and max(abs(a - b) for a, b in zip(l_on, l_off)) <= 1e-4 * max(l_off)
    assert any(bool((t.abs() == 0.02).any()) for t in rec[0]), "the clip value bites in this run"
    ref = R.run_torch("adam", p0, rec, torch.float64, lr=2e-3)[:3]          # the off arm's own gradients (already clipped), in fp64
    own = ([p.detach() for p in off.params], [off.optimizer.state[p]["exp_avg"] for p in off.params],
           [off.optimizer.state[p]["exp_avg_sq"] for p in off.params])
    shp = [tuple(p.shape) for p in on.params]
    got = ([p.detach() for p in on.params], R.split(on.optimizer._m, shp), R.split(on.optimizer._v, shp))
    _hold("adam", "driver", "hipgraph" if graph else "eager", got, own, ref)
    # a checkpoint saved by one resumes in the other, both ways
    off.save_checkpoint(); on.save_checkpoint()
    on2, off2 = _scheme(tmp_path, "off", True, graph, T, gpu), _scheme(tmp_path, "on", False, graph, T, gpu)
    assert on2.load_checkpoint() and off2.load_checkpoint()
    assert on2.optimizer.step_count() == 4 and on2.get_lr() == off.get_lr()
    _same_bits(own[1], R.split(on2.optimizer._m, shp), "m resumed from torch.optim's checkpoint")
    _same_bits(got[2], [off2.optimizer.state[p]["exp_avg_sq"] for p in off2.params], "v resumed from FlatOptimizer's checkpoint")
    assert all(float(off2.optimizer.state[p]["step"]) == 4.0 for p in off2.params)
    nxt = list(T.SyntheticZinc(32, 8, seed=2, pad_multiple=1))[:1]
    a, b = _train(on2, nxt), _train(off, nxt)
    assert abs(a[0] - b[0]) <= 1e-4 * abs(b[0])
    for x, y in zip(on2.params, off.params):
        assert float((x.detach() - y.detach()).abs().max()) <= 1e-5, "one more step from the same checkpoint"
