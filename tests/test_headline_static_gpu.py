"""k_block_fwd_s64 -- the forward pair kernel compiled for the ZINC-500K descriptor alone (N = 64, De = 64, d = 8, gate + clip,
training with the in-kernel random mask, 16-row groups) -- against the generic instance it replaces, and against the fp64 oracle.

The plan switches (EGT_NO_STATIC, EGT_FWD_ROWS, EGT_BWD_TL) are read once per process, so every variant runs in a fresh child process:
this file run as a script.  A child runs both cases through the C ABI and leaves its tensors in a temp directory:
  block   one block, egt_block_fwd / egt_block_bwd          (epilogue 1, backward prologue 1)
  stack   two layers, egt_stack_fwd / egt_stack_bwd         (epilogues 2 and 1, backward prologues 1 and 2)
at B = 4, N = 64, Dh = De = 64, H = 8, node counts [64, 37, 9, 0], random_mask_prob = 0.1, with EGT_FWD_ROWS = EGT_BWD_TL = 16 so that
the 16-row forms the headline batch takes are planned at this small one.  The checks:
  1. h', e', dh, de and the flat parameter-gradient buffer are the same bits with and without EGT_NO_STATIC=1;
  2. the default run holds util.FWD / util.BWD against the fp64 oracle (fed the masks the kernels draw: oracle/rng_ref.py);
  3. egt_block_plan_static answers 1 for these descriptors and 0 under EGT_NO_STATIC, for N = 48, without clip, with
     random_mask_prob = 0, and for B = 4 without the row overrides (four-row groups).
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

B, N, D, DE, H, DK = 4, 64, 64, 64, 8, 8
NODES = (64, 37, 9, 0)
PROB, SEED = 0.1, 0x5EED0064C0DE
CASES = {"block": 1, "stack": 2}          # layers
OUTPUTS = ("h_out", "e_out", "d_h", "d_e", "grads")
ROW_ENV = dict(EGT_FWD_ROWS="16", EGT_BWD_TL="16")


def make_desc(L, *, n=N, clip=True, prob=PROB):
    flags = L.BF_GATE | L.BF_TRAINING | (L.BF_CLIP if clip else 0)
    return L.BlockDesc(B=B, N=n, H=H, d=DK, De=DE, dtype=L.EGT_F32, flags=flags, clip_lo=-5.0, clip_hi=5.0,
                       random_mask_prob=prob, ln_eps=1e-3, reserved=0, seed=SEED, seed_device=None)


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """seeded host tensors of a case: dict(h, e, key_mask, dh, de, params: [layers][14])"""
    import memcontract as M
    from oracle import egt_oracle as O
    g = torch.Generator().manual_seed(6400 + CASES[case])
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    inp = dict(h=r(B, N, D), e=r(B, N, N, DE) * 1.3 + 0.2, dh=r(B, N, D), de=r(B, N, N, DE),
               key_mask=(torch.arange(N)[None, :] < torch.tensor(NODES)[:, None]).to(torch.uint8), params=[])
    for _ in range(CASES[case]):
        p = O.init_block_params(D, DE, H, dtype=torch.float32, generator=g, randomize_norm=True)
        inp["params"].append([p[k] for k in M.BLOCK_ORACLE_NAMES])
    return inp


# ------------------------------------------------------------------------------------------------------ the child process ----
def plan_answers(lib, L):
    q = lambda **kw: int(lib.egt_block_plan_static(C.byref(make_desc(L, **kw))))
    return dict(headline=q(), n48=q(n=48), no_clip=q(clip=False), prob0=q(prob=0.0), null=int(lib.egt_block_plan_static(None)))


def run_case(lib, L, case, dev):
    """the case through the C ABI: {name: tensor on the host}"""
    inp, layers = make_inputs(case), CASES[case]
    cu = lambda t: t.to(dev).contiguous()
    h, e, km, dh, de = (cu(inp[k]) for k in ("h", "e", "key_mask", "dh", "de"))
    params = [[cu(t) for t in lp] for lp in inp["params"]]
    sizes = [t.numel() for t in params[0]]
    grads = torch.full((layers * sum(sizes),), float("nan"), device=dev)
    gviews = [list(torch.split(grads[l * sum(sizes):(l + 1) * sum(sizes)], sizes)) for l in range(layers)]
    arr = lambda rows: (L.BlockParams * layers)(*[L.params_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, lp) for lp in rows])
    ptr = lambda t: C.c_void_p(t.data_ptr())
    desc = make_desc(L)
    d = C.byref(desc)
    stack = case == "stack"
    nb = (lambda f: f(d, layers)) if stack else (lambda f: f(d))
    saved = torch.zeros(nb(lib.egt_stack_saved_bytes if stack else lib.egt_block_saved_bytes), dtype=torch.uint8, device=dev)
    ws = torch.zeros(nb(lib.egt_stack_workspace_bytes if stack else lib.egt_block_workspace_bytes), dtype=torch.uint8, device=dev)
    h_out, e_out, d_h, d_e = torch.empty_like(h), torch.empty_like(e), torch.empty_like(h), torch.empty_like(e)
    st = L.current_stream()
    if stack:
        L.check(lib.egt_stack_fwd(d, layers, arr(params), ptr(h), ptr(e), ptr(km), None, ptr(h_out), ptr(e_out), ptr(saved), ptr(ws), st))
        L.check(lib.egt_stack_bwd(d, layers, arr(params), ptr(h), ptr(e), ptr(km), None, ptr(saved), ptr(dh), ptr(de), ptr(d_h), ptr(d_e),
                                  arr(gviews), ptr(ws), st))
    else:
        L.check(lib.egt_block_fwd(d, arr(params), ptr(h), ptr(e), ptr(km), None, None, ptr(h_out), ptr(e_out), ptr(saved), ptr(ws), st))
        L.check(lib.egt_block_bwd(d, arr(params), ptr(h), ptr(e), ptr(km), None, None, ptr(saved), ptr(dh), ptr(de), ptr(d_h), ptr(d_e),
                                  arr(gviews), ptr(ws), st))
    torch.cuda.synchronize()
    return dict(h_out=h_out.cpu(), e_out=e_out.cpu(), d_h=d_h.cpu(), d_e=d_e.cpu(), grads=grads.cpu())


def child_main(outdir, run):
    from egt_amd import _lib as L
    lib = L.load()
    res = dict(plan=plan_answers(lib, L), form=(lib.egt_block_launch_form(C.byref(make_desc(L))) or b"").decode())
    if run:
        dev = torch.device("cuda:0")
        for case in CASES:
            torch.save(run_case(lib, L, case, dev), os.path.join(outdir, case + ".pt"))
    with open(os.path.join(outdir, "plan.json"), "w") as f:
        json.dump(res, f)


# ------------------------------------------------------------------------------------------------------------- the tests ----
def _child(outdir, env_extra, run):
    env = {k: v for k, v in os.environ.items() if k not in ("EGT_NO_STATIC", "EGT_FWD_ROWS", "EGT_BWD_TL")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), outdir, "run" if run else "plan"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child {env_extra} failed:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    out = json.load(open(os.path.join(outdir, "plan.json")))
    if run:
        out.update({case: torch.load(os.path.join(outdir, case + ".pt")) for case in CASES})
    return out


@pytest.fixture(scope="module")
def runs(gpu, egt_lib):
    """{variant: {plan, form, block: {...}, stack: {...}}} of the default and the EGT_NO_STATIC=1 child, and the plan answers of a
    child without the row overrides"""
    with tempfile.TemporaryDirectory() as tmp:
        out = {}
        for name, env, run in (("static", ROW_ENV, True), ("generic", dict(ROW_ENV, EGT_NO_STATIC="1"), True), ("no_rows", {}, False)):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            out[name] = _child(d, env, run)
    return out


@functools.lru_cache(maxsize=None)
def oracle(case):
    """fp64 oracle of a case, fed the masks the kernels draw: the call's seed for a block call, layer_seed() of it in a stack"""
    import memcontract as M
    from oracle import egt_oracle as O, rng_ref
    inp, layers = make_inputs(case), CASES[case]
    seeds = [SEED] if case == "block" else [M.layer_seed(SEED, l) for l in range(layers)]
    rms = [torch.from_numpy(rng_ref.random_mask(s, B, N, H, PROB)) for s in seeds]
    h = inp["h"].double().requires_grad_()
    e = inp["e"].double().requires_grad_()
    ps = [{k: t.double().requires_grad_() for k, t in zip(M.BLOCK_ORACLE_NAMES, lp)} for lp in inp["params"]]
    h2, e2 = O.stack_forward(h, e, inp["key_mask"].bool(), ps, rand_masks=rms, num_heads=H)
    flat = [t for lp in ps for t in lp.values()]
    gr = torch.autograd.grad([h2, e2], [h, e] + flat, [inp["dh"].double(), inp["de"].double()])
    return dict(h_out=h2.detach(), e_out=e2.detach(), d_h=gr[0], d_e=gr[1], grads=list(gr[2:]))


@pytest.mark.parametrize("case", list(CASES))
def test_static_equals_generic_bits(case, runs):
    assert runs["static"]["plan"]["headline"] == 1 and runs["generic"]["plan"]["headline"] == 0
    assert runs["static"]["form"] == runs["generic"]["form"] == "fwd=k_block_fwd/4w bwd=k_block_bwd_v5/4w/tl16"
    a, b = runs["static"][case], runs["generic"][case]
    for k in OUTPUTS:
        assert torch.isfinite(a[k]).all(), f"{case}: {k} has non-finite values"
        assert torch.equal(a[k], b[k]), f"{case}: {k} differs in {int((a[k] != b[k]).sum())} of {a[k].numel()} elements under EGT_NO_STATIC=1"


@pytest.mark.parametrize("case", list(CASES))
def test_static_vs_oracle(case, runs):
    import memcontract as M
    from util import BWD, FWD, assert_close, margin
    got, ref = runs["static"][case], oracle(case)
    sizes = [t.numel() for t in make_inputs(case)["params"][0]] * CASES[case]
    pairs = [(k, got[k], ref[k], k.startswith("d_")) for k in ("h_out", "e_out", "d_h", "d_e")]
    for i, (g, r) in enumerate(zip(torch.split(got["grads"], sizes), ref["grads"])):
        pairs.append((f"L{i // 14}.{M.BLOCK_ORACLE_NAMES[i % 14]}", g.reshape(r.shape), r, True))
    for name, g, r, is_grad in pairs:
        tol = BWD if is_grad else FWD
        if float(r.abs().max()) >= 1e-9:
            print(f"{case}: {name} margin {margin(g, r, rtol=tol['rtol'], arel=tol['arel']):.3f}")
        assert_close(g, r, name=f"{case}: {name}", **tol)


def test_plan_static_answers(runs):
    assert runs["static"]["plan"] == dict(headline=1, n48=0, no_clip=0, prob0=0, null=0)
    assert set(runs["generic"]["plan"].values()) == {0}                       # EGT_NO_STATIC=1
    assert set(runs["no_rows"]["plan"].values()) == {0}                       # B = 4 plans four-row groups
    assert "tl16" not in runs["no_rows"]["form"]


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2] == "run")
