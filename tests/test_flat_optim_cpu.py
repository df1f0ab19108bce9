"""Fused flat optimizer without a GPU: exports and struct layouts, the argument checks of the two entry points, the
work-item planner, the state-dict conversions against real torch.optim state dicts, and the config key."""
import copy
import ctypes as C
import os
import subprocess

import pytest
import torch

import optim_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_struct_layout(egt_lib, tmp_path):
    from egt_amd import _lib as L
    header = open(os.path.join(REPO, "include", "egt_amd.h")).read()
    for name in ("egt_optim_supported", "egt_optim_prepare", "egt_optim_step"):
        assert name in L._PROTOS and getattr(egt_lib, name) is not None and f"int {name}(" in header
    assert L.ABI_VERSION == 4 and egt_lib.egt_abi_version() == 4 and "#define EGT_ABI_VERSION 4" in header
    pairs = [("egt_optim_desc", L.OptimDesc), ("egt_optim_segment", L.OptimSegment)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "egt_amd.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("consts %d\\n", EGT_OPT_ADAM * 10000 + EGT_OPT_RMSPROP * 1000 + EGT_OPT_SGD * 100 + (int)EGT_OPT_CLIP * 10 + (int)EGT_OPT_ZERO_GRAD);',
              '  printf("state %d\\n", EGT_OPTIM_STATE_BYTES);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert C.sizeof(L.OptimSegment) == 24
    assert int(got["consts"]) == L.OPT_ADAM * 10000 + L.OPT_RMSPROP * 1000 + L.OPT_SGD * 100 + L.OPT_CLIP * 10 + L.OPT_ZERO_GRAD
    assert int(got["state"]) == L.OPTIM_STATE_BYTES


def _desc(L, **kw):
    d = dict(algo=L.OPT_ADAM, flags=0, num_segments=3, reserved=0, total=100, beta1=0.9, beta2=0.999, eps=1e-7, clip_value=0.0)
    d.update(kw)
    return L.OptimDesc(**d)


def test_argument_checks_return_the_documented_codes_without_launching(egt_lib):
    from egt_amd import _lib as L
    one = C.c_void_p(64)                                      # non-NULL, 16-byte aligned, never dereferenced here

    def prep(d, state=one):
        return egt_lib.egt_optim_prepare(C.byref(d) if d is not None else None, state, None)

    def step(d, table=one, grad=one, m=one, v=one, state=one):
        return egt_lib.egt_optim_step(C.byref(d) if d is not None else None, table, grad, m, v, state, None)

    ok = _desc(L)
    assert egt_lib.egt_optim_supported(C.byref(ok)) == 1
    assert prep(None) == L.EGT_E_NULL and step(None) == L.EGT_E_NULL and egt_lib.egt_optim_supported(None) == 0
    assert prep(ok, state=None) == L.EGT_E_NULL
    for k in ("table", "grad", "m", "v", "state"):
        assert step(ok, **{k: None}) == L.EGT_E_NULL, k
    assert b"state" in egt_lib.egt_last_error_string()
    assert step(_desc(L, algo=L.OPT_RMSPROP), v=None) == L.EGT_E_NULL and step(_desc(L, algo=L.OPT_RMSPROP), table=None, m=None) == L.EGT_E_NULL
    assert step(_desc(L, algo=L.OPT_SGD), grad=None, m=None, v=None) == L.EGT_E_NULL and b"grad" in egt_lib.egt_last_error_string()
    for bad, code in ((dict(algo=3), L.EGT_E_FLAGS), (dict(algo=-1), L.EGT_E_FLAGS), (dict(flags=0x4), L.EGT_E_FLAGS),
                      (dict(reserved=1), L.EGT_E_FLAGS), (dict(flags=L.OPT_CLIP, clip_value=0.0), L.EGT_E_FLAGS),
                      (dict(flags=L.OPT_CLIP, clip_value=float("nan")), L.EGT_E_FLAGS),
                      (dict(num_segments=0), L.EGT_E_SHAPE), (dict(total=2), L.EGT_E_SHAPE), (dict(beta1=1.0), L.EGT_E_SHAPE),
                      (dict(beta2=-0.1), L.EGT_E_SHAPE), (dict(eps=-1.0), L.EGT_E_SHAPE)):
        d = _desc(L, **bad)
        assert prep(d) == code and step(d) == code and egt_lib.egt_optim_supported(C.byref(d)) == 0, bad
    assert step(ok, grad=C.c_void_p(68)) == L.EGT_E_SHAPE and b"16-byte" in egt_lib.egt_last_error_string()
    assert step(_desc(L, algo=L.OPT_SGD), m=C.c_void_p(4), v=C.c_void_p(4), table=None) == L.EGT_E_NULL   # ignored pointers are not inspected
    for algo in (L.OPT_ADAM, L.OPT_RMSPROP, L.OPT_SGD):
        for flags in (0, L.OPT_CLIP, L.OPT_ZERO_GRAD, L.OPT_CLIP | L.OPT_ZERO_GRAD):
            assert egt_lib.egt_optim_supported(C.byref(_desc(L, algo=algo, flags=flags, clip_value=0.5))) == 1


@pytest.mark.parametrize("numels", [R.RAGGED, (1,), (2048,), (2049,), (1, 1, 1), (0, 5, 0), (4096, 1, 6145)])
def test_planner_covers_every_element_once_and_never_straddles(numels):
    from egt_amd.optim import ITEM, plan_items
    items = plan_items(numels)
    starts = [sum(numels[:i]) for i in range(len(numels))]
    nxt = 0
    for i, s, off, cnt in items:
        assert 1 <= cnt <= ITEM and 0 <= s and s + cnt <= numels[i], "inside one parameter"
        assert off == starts[i] + s and off == nxt, "flat order, no gap, no overlap"
        nxt = off + cnt
    assert nxt == sum(numels)
    if numels == R.RAGGED:
        assert [c for i, _, _, c in items if i == 4] == [2048, 1] and [c for i, _, _, c in items if i == 5] == [2048, 2048, 5]
        assert [c for i, _, _, c in items if i < 3] == [1, 3, 7]
    assert len(plan_items(numels, item=3)) == sum(-(-n // 3) for n in numels)
    with pytest.raises(ValueError):
        plan_items((3, -1))


@pytest.mark.parametrize("algo", R.ALGOS)
def test_state_dict_conversions_round_trip_torch_optim(algo):
    from egt_amd.optim import flat_to_state, state_to_flat
    p0, g = R.params0("ragged"), R.grads("ragged", "normal")
    ps, m, v, opt = R.run_torch(algo, p0, g[:3], torch.float32)
    sd = opt.state_dict()
    shp = [tuple(p.shape) for p in ps]
    n = sum(p.numel() for p in ps)
    fm = torch.full((n,), 7.0) if algo == "adam" else None
    fv = torch.full((n,), 7.0) if algo != "sgd" else None
    step = state_to_flat(algo, sd["state"], shp, fm, fv)
    assert step == (0 if algo == "sgd" else 3)
    if fm is not None:
        assert torch.equal(fm, torch.cat([x.reshape(-1) for x in m]))
    if fv is not None:
        assert torch.equal(fv, torch.cat([x.reshape(-1) for x in v]))
    back = flat_to_state(algo, shp, step, fm, fv)
    assert set(back) == set(sd["state"])
    for i, d in sd["state"].items():
        assert set(back[i]) == set(d)
        for k, t in d.items():
            assert back[i][k].dtype == t.dtype and back[i][k].shape == t.shape and torch.equal(back[i][k], t), (i, k)
    # torch loads what the conversion produced, and continues exactly as the optimizer it came from
    ps2 = [torch.nn.Parameter(p.clone()) for p in ps]
    o2 = R.torch_optimizer(algo, ps2)
    o2.load_state_dict({"state": back, "param_groups": sd["param_groups"]})
    for q, gr in zip(ps2, g[3]):
        q.grad = gr.clone()
    cont = R.run_torch(algo, ps, g[3:4], torch.float32, state=sd)[0]
    o2.step()
    for a, b in zip(cont, ps2):
        assert torch.equal(a, b.detach())
    # a fresh optimizer: empty state both ways
    assert flat_to_state(algo, shp, 0, fm, fv) == {} == R.torch_optimizer(algo, ps2).state_dict()["state"]
    if fv is not None:
        assert state_to_flat(algo, {}, shp, fm, fv) == 0 and float(fv.abs().max()) == 0.0


def test_unequal_steps_and_foreign_state_are_refused():
    from egt_amd.optim import state_to_flat
    p0, g = R.params0("ragged"), R.grads("ragged", "normal")
    ps, _, _, opt = R.run_torch("adam", p0, g[:2], torch.float32)
    shp = [tuple(p.shape) for p in ps]
    n = sum(p.numel() for p in ps)
    fm, fv = torch.zeros(n), torch.zeros(n)
    sd = copy.deepcopy(opt.state_dict())               # (state_dict() hands out the optimizer's own per-parameter dicts)
    sd["state"][2]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="one counter"):
        state_to_flat("adam", sd["state"], shp, fm, fv)
    sd = copy.deepcopy(opt.state_dict())
    del sd["state"][0]
    with pytest.raises(ValueError, match="all or none"):
        state_to_flat("adam", sd["state"], shp, fm, fv)
    with pytest.raises(ValueError):
        state_to_flat("rmsprop", opt.state_dict()["state"], shp, None, fv)             # Adam's moments are not RMSprop's
    ams = R.run_torch("adam", p0, g[:1], torch.float32, amsgrad=True)[3].state_dict()
    with pytest.raises(ValueError, match="max_exp_avg_sq"):
        state_to_flat("adam", ams["state"], shp, fm, fv)
    mom = torch.optim.SGD([torch.nn.Parameter(p.clone()) for p in p0], lr=0.1, momentum=0.9)
    for p in mom.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    mom.step()
    with pytest.raises(ValueError, match="momentum"):
        state_to_flat("sgd", mom.state_dict()["state"], shp)
    bad = copy.deepcopy(opt.state_dict())
    bad["state"][1]["exp_avg"] = torch.zeros(4)
    with pytest.raises(ValueError, match="shape"):
        state_to_flat("adam", bad["state"], shp, fm, fv)


def test_config_key_and_the_cpu_refusal(tmp_path):
    import egt_amd.training as T
    assert T.default_config()["fused_optimizer"] is False
    c = T.make_config({"fused_optimizer": True})
    assert c.fused_optimizer is True and c.use_hipgraph is False
    for scheme in T.SCHEMES:
        assert T.make_config({"scheme": scheme}).fused_optimizer is False
    cfg = dict(scheme="zinc.svd", model_width=16, edge_width=16, model_height=1, use_svd=False, fused_optimizer=True,
               save_path=str(tmp_path / "run"))
    with pytest.raises(ValueError, match="fused_optimizer needs"):
        T.ZincSVDScheme(cfg, device=None).load_model()
    with pytest.raises(ValueError, match="fused_optimizer needs"):
        T.ZincSVDScheme(cfg, device="cpu").load_model()


def test_flat_optimizer_refuses_cpu_parameters_at_construction():
    from egt_amd import FlatOptimizer
    from egt_amd.dp import FlatGradAllReduce
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(5))]
    flat = FlatGradAllReduce(ps, direct=True)
    with pytest.raises(ValueError, match="on a GPU"):
        FlatOptimizer(ps, flat)
    with pytest.raises(ValueError, match="in its order"):
        FlatOptimizer(ps[::-1], flat)
    with pytest.raises(ValueError, match="algo"):
        FlatOptimizer(ps, flat, algo="lamb")


def test_fixture_sets_are_the_issues():
    assert [R.numel(s) for s in R.shapes("ragged")] == [1, 3, 7, 64, 2049, 4101]
    z = [R.numel(s) for s in R.shapes("zinc16")]
    assert len(z) > 20 and min(z) == 1 and max(z) < 2048, "a real model's list: many small tensors, every one a single work item"
    g = R.grads("ragged", "clipped")
    allv = torch.cat([t.reshape(-1) for t in g[0]])
    assert bool((allv.abs() > R.CLIP).any()) and bool((allv.abs() < R.CLIP).any())
    assert float(torch.tensor(1e-18, dtype=torch.float32) ** 2 * 0.001) < 1.1754944e-38        # subnormal second moment
    assert not torch.isfinite(torch.tensor(1e20, dtype=torch.float32) ** 2)
