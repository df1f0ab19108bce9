"""config.resident_step on the GPU (egt_amd/graph.py: ResidentStep, DeviceAccumulator; csrc/egt_batch.hip, csrc/egt_accum.hip).

Entry points: egt_batch_assemble_at equals egt_batch_assemble on the same indices and reads its table and cursor only;
egt_accumulate keeps the fp64 sums a host loop keeps, eager and replayed from a hipGraph.
Driver: with use_hipgraph, fused_optimizer and device_dataset on, turning resident_step on changes no bit of the parameters,
of Adam's moments and step count, of any metric sum or validation figure; the epoch's loss mean is the accumulator's
sequential fp64 sum / n against np.mean's pairwise one, so it is held to the reordering bound n 2^-52 max|loss_i|.
The stores are the 13 graphs of tests/device_data_cases.py (clean_records)."""
import numpy as np
import pytest
import torch

import device_data_cases as DC
from egt_amd import data as D

pytestmark = pytest.mark.gpu
FAMILIES = [(name, level) for name, levels in DC.LEVELS.items() for level in levels]


# ------------------------------------------------------------------------------------------------ entry points -----
def _device_set(tmp_path, name, level, gpu):
    path = DC.write_store(tmp_path, name, DC.clean_records(name, 0), DC.clean_records(name, 1)[:5])
    kw = dict(level=level, max_length=None, max_shuffle_len=6, seed=3, prefetch_batch=False, num_features=4)
    if level == "svd":
        kw["return_mat"] = True
    return D.GraphDataset(name, path, **kw).to_device(gpu)


@pytest.mark.parametrize("name,level", FAMILIES)
def test_assemble_at_equals_assemble(name, level, tmp_path, gpu, egt_lib):
    from egt_amd.device_data import assemble_batch, batch_desc
    dev = _device_set(tmp_path, name, level, gpu)
    sp = dev._splits["training"]
    order = np.random.default_rng(5).permutation(13).astype(np.int32)
    table = torch.from_numpy(order).to(gpu)
    table0 = table.clone()
    fields = [f for _, f in dev.batch_keys("training")]
    odd = 0
    for cur, B in ((0, 4), (5, 4), (12, 1)):               # the table's start, its middle, the short last batch of 13 = 3 x 4 + 1
        ids = order[cur:cur + B]
        N = int(sp.num_nodes_host[ids].max())
        odd += N % 4 != 0
        desc = batch_desc(sp.kinds, B, N, sp.records)
        ref = assemble_batch(desc, sp.store, torch.from_numpy(ids.copy()).to(gpu), fields)
        cursor = torch.tensor([cur], dtype=torch.int64, device=gpu)
        out = {f: torch.empty_like(t).view(torch.uint8).fill_(0xFF).view(t.dtype).view(t.shape) for f, t in ref.items()}
        got = assemble_batch(desc, sp.store, table, fields, out=out, cursor=cursor)
        torch.cuda.synchronize()
        assert set(got) == set(ref) == set(fields)
        for f in fields:
            assert got[f] is out[f] and got[f].dtype == ref[f].dtype and got[f].shape == ref[f].shape
            assert torch.equal(got[f].view(torch.int32), ref[f].view(torch.int32)), (f, cur, B)
        assert int(cursor.item()) == cur and torch.equal(table, table0), "the cursor and the table are only read"
    assert odd >= 1, "one batch with N not a multiple of 4"


def _acc_setup(gpu, K, counts):
    """K items over a [2K] fp32 value buffer; item k has a count pointer iff counts[k] is None"""
    from egt_amd import _lib as L
    vals = torch.zeros(2 * K, dtype=torch.float32, device=gpu)
    items = (L.AccItem * K)()
    for k in range(K):
        items[k].sum = vals.data_ptr() + 8 * k
        items[k].count = vals.data_ptr() + 8 * k + 4 if counts[k] is None else None
        items[k].count_value = 0.0 if counts[k] is None else counts[k]
    dev_items = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(gpu)
    return vals, dev_items


def _steps(n, K, seed=0):
    """n steps of K (sum, count) fp32 pairs whose fp64 running sums depend on the order of the additions"""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((n, 2 * K)) * 10.0 ** rng.integers(-6, 7, size=(n, 2 * K))).astype(np.float32)
    v[:, 1::2] = np.abs(v[:, 1::2])
    return v


def test_accumulate_equals_sequential_host_additions(gpu, egt_lib):
    from egt_amd import _lib as L
    K, n = 3, 50
    counts = [None, 7.0, None]                             # the middle item counts by its constant
    vals, items = _acc_setup(gpu, K, counts)
    acc = torch.zeros(2 * K + 2, dtype=torch.float64, device=gpu)
    acc[-2:] = 123.25                                      # two words past acc[0 .. 2K): not the kernel's
    steps = _steps(n, K)
    want = np.zeros(2 * K, np.float64)
    for s in steps:
        vals.copy_(torch.from_numpy(s))
        L.check(egt_lib.egt_accumulate(L.ptr(acc), L.ptr(items), K, L.current_stream()))
        for k in range(K):
            want[2 * k] += float(s[2 * k])
            want[2 * k + 1] += float(s[2 * k + 1]) if counts[k] is None else counts[k]
    got = acc.cpu().numpy()
    assert got[:2 * K].tobytes() == want.tobytes(), (got[:2 * K], want)
    assert got[-2:].tolist() == [123.25, 123.25]
    assert torch.equal(vals.cpu(), torch.from_numpy(steps[-1])), "the items' values are only read"


def test_accumulate_replayed_equals_eager(gpu, egt_lib):
    from egt_amd import _lib as L
    K, n = 3, 12
    vals, items = _acc_setup(gpu, K, [None, 2.0, None])
    src = torch.from_numpy(_steps(n, K, 1)).to(gpu)
    row = torch.zeros((), dtype=torch.int64, device=gpu)
    eager, replayed = (torch.zeros(2 * K, dtype=torch.float64, device=gpu) for _ in range(2))

    def step(acc):
        vals.copy_(src.index_select(0, row.reshape(1)).reshape(-1))
        L.check(egt_lib.egt_accumulate(L.ptr(acc), L.ptr(items), K, L.current_stream()))
        row.add_(1)
    for _ in range(n):
        step(eager)
    torch.cuda.synchronize()
    row.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(replayed)
    for _ in range(n):
        graph.replay()
    torch.cuda.synchronize()
    assert int(row.item()) == n
    assert torch.equal(eager, replayed) and float(eager.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------------ driver -----
EPOCH_SEED = 100          # epoch e of every run draws its order from default_rng(EPOCH_SEED + e): runs and resumed runs agree


def _case(which):
    from egt_amd import training as T
    base = dict(num_epochs=0, initial_lr=2e-3, batch_size=4, upto_hop=4, model_height=2, save_best=False, num_svd_features=8,
                sel_svd_features=4, use_hipgraph=True, fused_optimizer=True, device_dataset=True)
    if which.startswith("zinc"):
        cfg = dict(base, scheme="zinc.svd", model_width=64, edge_width=64, random_mask_prob=0.1)
        if which == "zinc_warmup":
            cfg.update(warmup_steps=5, total_steps=40)      # the rate changes on every step: warm-up, then the cosine (no epoch ends at its peak)
        if which == "zinc_distance":
            cfg.update(distance_loss=0.05, distance_target=3)
        if which == "zinc_plain":      # no random draws at all: a capture's warm-up discards a mask sample and the sign draw of the SVD
            cfg.update(random_mask_prob=0.0, use_svd=False)   # encoding comes from torch's generator, which no checkpoint holds
        return T.ZincSVDScheme, "zinc", cfg
    return T.PatternSVDScheme, "sbm_pattern", dict(base, scheme="pattern.svd", model_width=64, edge_width=8)


def _make(which, gpu, tmp_path, tag, resident):
    cls, name, cfg = _case(which)
    store = str(tmp_path / f"{name}.npz")
    if not (tmp_path / f"{name}.npz").exists():
        DC.write_store(tmp_path, name, DC.clean_records(name, 0), DC.clean_records(name, 1)[:5])
    torch.manual_seed(0)
    s = cls(dict(cfg, model_name=tag, save_path=str(tmp_path / tag), dataset_path=store, resident_step=resident), device=gpu,
            print_fn=lambda *a: None)
    s.load_data()
    s.dataset.prefetch_batch = False
    s.load_model()
    s.load_state()
    return s


def _snapshot(s):
    o = s.optimizer
    return dict(params=[p.detach().clone() for p in s.params], m=None if o._m is None else o._m.clone(), v=o._v.clone(),
                step=o.step_count(), logs=dict(s.history[-1]), sums={k: list(v) for k, v in s.epoch_sums.items()})


def _epoch(s, e, seed=None):
    """epoch e (1-based) of scheme s; the off path's per-step losses are kept for the loss bound"""
    s.dataset._rng = np.random.default_rng(EPOCH_SEED + e if seed is None else seed)
    step, losses = s.train_step, []
    if not s.config.resident_step:
        s.train_step = lambda b: (losses.append(step(b)), losses[-1])[1]
    s.config["num_epochs"] = e
    try:
        s.train_model()
    finally:
        s.train_step = step
    assert s.state.current_epoch == e
    return dict(_snapshot(s), losses=losses)


def _same_state(a, b, where):
    for i, (x, y) in enumerate(zip(a["params"], b["params"])):
        assert torch.equal(x, y), (where, "parameter", i)
    assert (a["m"] is None) == (b["m"] is None) and (a["m"] is None or torch.equal(a["m"], b["m"])), (where, "m")
    assert torch.equal(a["v"], b["v"]), (where, "v")
    assert a["step"] == b["step"] > 0, (where, "step count", a["step"], b["step"])


def _compare(off, on, where):
    _same_state(off, on, where)
    assert off["sums"] == on["sums"], (where, off["sums"], on["sums"])                 # fp64 sums of the same fp32 values, same order
    n, big = len(off["losses"]), max(abs(x) for x in off["losses"])
    assert n == 4                                                                     # 13 graphs in batches of 4
    assert off["logs"]["loss"] == float(np.mean(off["losses"]))
    bound = n * 2.0 ** -52 * big
    err = abs(on["logs"]["loss"] - off["logs"]["loss"])
    print(f"{where}: loss mean on {on['logs']['loss']!r} off {off['logs']['loss']!r} |diff| {err:.3e} bound {bound:.3e}")
    assert err <= bound, (where, err, bound)
    assert set(off["logs"]) == set(on["logs"]) and any(k.startswith("val_") for k in off["logs"])
    for k, v in off["logs"].items():                       # lr, the training metrics, every validation figure
        if k != "loss" and v != off["logs"]["loss"]:       # (logs[LOSS_METRIC] repeats the loss: held to the bound above)
            assert v == on["logs"][k], (where, k, v, on["logs"][k])


@pytest.mark.parametrize("which", ["zinc", "pattern", "zinc_warmup", "zinc_distance"])
def test_resident_step_changes_no_bit_of_the_run(which, tmp_path, gpu, egt_lib):
    # one run after the other, each from torch.manual_seed(0): the SVD encoding's sign draw comes from torch's generator
    off = _make(which, gpu, tmp_path, "off", False)
    offs = [_epoch(off, e) for e in (1, 2, 3)]
    on = _make(which, gpu, tmp_path, "on", True)
    assert on._resident and not off._resident
    captures = []
    for e, a in zip((1, 2, 3), offs):
        b = _epoch(on, e)
        _compare(a, b, f"{which} epoch {e}")
        captures.append(on._resident_captures)
        if which == "zinc_distance":
            assert set(b["sums"]) == {"mae", "distance_loss"} and b["sums"]["distance_loss"][1] == 13.0
        if which == "zinc_warmup":
            assert b["logs"]["lr"] == a["logs"]["lr"] != on.config.initial_lr
    steps = [ent[1].replays for ent in on._graphs.values()]
    print(f"{which}: captures after each epoch {captures}, replays per geometry {steps}")
    assert sum(steps) == 12 and on.state.global_step == off.state.global_step == 12
    assert max(steps) >= 2, "a geometry was replayed from the cache"
    assert captures[-1] > captures[0], "a geometry was captured after the first epoch"
    assert torch.is_tensor(on.train_step(next(iter(on.trainset)))) and on._graphs
    on.release_graphs(); off.release_graphs()
    assert not on._graphs


def test_warm_steps_and_an_evaluation_pass_do_not_synchronise(tmp_path, gpu, egt_lib):
    """a second epoch in the first one's order (every geometry warm) and one evaluation pass under
    torch.cuda.set_sync_debug_mode("error"): only the two read-backs, one per epoch and one per pass, sit outside"""
    s = _make("zinc_warmup", gpu, tmp_path, "on", True)
    first = _epoch(s, 1, seed=EPOCH_SEED)
    captured = s._resident_captures
    s.dataset._rng = np.random.default_rng(EPOCH_SEED)
    s._train_acc.zero()
    s.evaluate(s.valset)                                   # (the eager forward's lazy one-time work)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=gpu).item()
            inert = True
        except RuntimeError:
            inert = False
        losses = [s.train_step(b) for b in s.trainset]
        keys, dacc = s.evaluate_on_device(s.valset)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("torch.cuda.set_sync_debug_mode('error') is " + ("INERT in this build: a .item() passed; the region ran unguarded" if inert
                                                            else "live: a .item() raised inside the region"))
    assert s._resident_captures == captured and len(losses) == 4 and all(t.is_cuda and t.dim() == 0 for t in losses)
    got, val = s._train_acc.read(), dict(zip(keys, dacc.read()))
    assert got[0][1] == 4.0 and np.isfinite(got[0][0]) and np.isfinite(first["logs"]["loss"])
    assert val["mae"][1] == 5.0 and np.isfinite(val["mae"][0])
    s.release_graphs()


def _restored(part, resumed, where):
    o, r = part.optimizer, resumed.optimizer
    for i, (x, y) in enumerate(zip(part.params, resumed.params)):
        assert torch.equal(x, y), (where, "parameter", i)
    assert torch.equal(o._m, r._m) and torch.equal(o._v, r._v) and o.step_count() == r.step_count() == 8, where
    assert resumed.state.current_epoch == 2 and resumed.state.global_step == 8
    if part._seeds is not None:
        assert part._seeds.values() == resumed._seeds.values(), (where, "mask seeds")


def test_a_resumed_run_continues_the_uninterrupted_one(tmp_path, gpu, egt_lib):
    """A checkpoint written at an epoch's end, resumed in a new scheme object.  `zinc_plain` (no random mask, no SVD sign draw)
    must CONTINUE bit-equal to the uninterrupted run.  That part is narrowed to a model that draws nothing at random, because
    two things outside this key stand between a drawing model and a bit-equal continuation, with the key on as with it off: a
    resumed run captures its geometries again and every capture's warm-up discards one mask sample, and torch's generator (the
    SVD encoding's sign draw) is in no checkpoint.  What does hold for the drawing `zinc` model is asserted too: parameters,
    Adam's m, v and step count, the counters and the device mask seeds are restored exactly at the resume point."""
    whole = _make("zinc_plain", gpu, tmp_path, "whole", True)
    for e in (1, 2, 3):
        ref = _epoch(whole, e)
    part = _make("zinc_plain", gpu, tmp_path, "part", True)
    for e in (1, 2):
        _epoch(part, e)                                    # train_model writes the checkpoint at every epoch's end
    resumed = _make("zinc_plain", gpu, tmp_path, "part", True)   # a new scheme object over the same save_path: load_state restores
    _restored(part, resumed, "zinc_plain")
    got = _epoch(resumed, 3)
    _same_state(ref, got, "resumed epoch 3")
    assert ref["logs"]["loss"] == got["logs"]["loss"] and ref["logs"]["val_mae"] == got["logs"]["val_mae"]
    whole.release_graphs(); part.release_graphs(); resumed.release_graphs()
    drawing = _make("zinc", gpu, tmp_path, "draw", True)
    for e in (1, 2):
        _epoch(drawing, e)
    again = _make("zinc", gpu, tmp_path, "draw", True)
    _restored(drawing, again, "zinc")
    drawing.release_graphs(); again.release_graphs()
