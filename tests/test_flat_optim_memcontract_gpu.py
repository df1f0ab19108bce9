"""egt_optim_prepare / egt_optim_step under the memory-contract harness (tests/memcontract.py): every parameter, the flat
buffers, the table and the state block in guarded arenas of exactly their byte count, the parameters shifted to 4-byte
alignment, m / v NULL where the algorithm ignores them; the result bit for bit the Python wrapper's."""
import ctypes as C
import struct

import pytest
import torch

import memcontract as MC
import optim_ref as R

pytestmark = pytest.mark.gpu
STEPS = 2
CASES = [(a, f) for a in R.ALGOS for f in ("plain", "clip_zero")]


def _case(lib, algo, form):
    from egt_amd import _lib as L
    from egt_amd.optim import plan_items
    p0, g = R.params0("ragged"), R.grads("ragged", "clipped")[0]
    numels = [p.numel() for p in p0]
    total = sum(numels)
    items = plan_items(numels)
    zero = form == "clip_zero"
    flags = (L.OPT_CLIP | L.OPT_ZERO_GRAD) if zero else 0
    desc = L.OptimDesc(algo=R.ALGOS.index(algo), flags=flags, num_segments=len(items), reserved=0, total=total,
                       beta1=0.9 if algo == "adam" else 0.0, beta2=0.999 if algo == "adam" else 0.9, eps=1e-7,
                       clip_value=R.CLIP if zero else 0.0)
    d = C.byref(desc)
    state0 = torch.frombuffer(bytearray(struct.pack("<qdfi", 0, R.LR, 1.0, 0) + bytes(L.OPTIM_STATE_BYTES - 24)), dtype=torch.uint8)
    bufs = [MC.Buf(f"p{i}", MC.INOUT, p) for i, p in enumerate(p0)]
    bufs.append(MC.Buf("grad", MC.INOUT if zero else MC.IN, torch.cat([t.reshape(-1) for t in g])))
    if algo == "adam":
        bufs.append(MC.Buf("m", MC.INOUT, torch.zeros(total)))
    if algo != "sgd":
        bufs.append(MC.Buf("v", MC.INOUT, torch.zeros(total)))
    bufs += [MC.Buf("state", MC.INOUT, state0),
             MC.Buf("table", MC.CARRIED, dtype=torch.int64, shape=(len(items), 3), const_after=0)]      # exactly 24 bytes per item

    def write_table(v):                       # the host's part: the addresses are known once the arenas exist
        host = torch.tensor([[v[f"p{i}"].data_ptr() + 4 * s, off, cnt] for i, s, off, cnt in items], dtype=torch.int64)
        v["table"].copy_(host)
        return 0

    def prepare(v):
        return lib.egt_optim_prepare(d, MC._ptr(v, "state"), MC._stream())

    def step(v):
        return lib.egt_optim_step(d, MC._ptr(v, "table"), MC._ptr(v, "grad"), MC._ptr(v, "m"), MC._ptr(v, "v"), MC._ptr(v, "state"),
                                  MC._stream())
    return MC.Case(f"optim_{algo}_{form}", bufs, [write_table] + [prepare, step] * STEPS), p0, g


@pytest.mark.parametrize("algo,form", CASES, ids=[f"{a}-{f}" for a, f in CASES])
def test_optim_entry_points_keep_the_buffer_contract(algo, form, gpu, egt_lib):
    from egt_amd import _lib as L
    case, p0, g = _case(egt_lib, algo, form)
    kw = dict(sync=torch.cuda.synchronize, check_rc=L.check)
    z = MC.run(case, MC.ZERO, gpu, **kw)
    p = MC.run(case, MC.POISON, gpu, **kw)
    MC.assert_finite(case, p)
    MC.assert_same_bits(case, z, p)
    for which, shift in (("all", {f"p{i}": 4 * (1 + i % 3) for i in range(len(p0))}),
                         ("mixed", {f"p{i}": 4 * (1 + i % 3) for i in range(len(p0)) if i % 4 in (0, 3)})):
        u = MC.run(case, MC.POISON, gpu, shift=shift, **kw)
        MC.assert_same_bits(case, z, u, names=("Z", f"U-{which}"))
        MC.assert_finite(case, u, f"U-{which}")
    # the Python wrapper, bit for bit (under EGT_OPT_ZERO_GRAD the second step of the sequence sees the zeroed gradients)
    zero = form == "clip_zero"
    gsteps = [g] + [tuple(torch.zeros_like(t) for t in g) if zero else g] * (STEPS - 1)
    w = R.run_flat(algo, p0, gsteps, gpu, clip=R.CLIP if zero else None, zero_grad=zero)
    for i, t in enumerate(w[0]):
        assert torch.equal(t.view(torch.int32), z[f"p{i}"].view(torch.int32)), f"p{i}"
    shp = [tuple(t.shape) for t in p0]
    for name, flat in (("m", w[3]._m), ("v", w[3]._v)):
        if flat is not None:
            assert torch.equal(flat.view(torch.int32), z[name].view(torch.int32)), name
    assert torch.equal(w[3]._state.cpu(), z["state"].cpu()), "the state block"
    if zero:
        assert float(z["grad"].abs().max()) == 0.0
