"""config.resident_step without a GPU: the two C-ABI entries it adds (egt_batch_assemble_at, egt_accumulate) are declared,
exported and validate their arguments before any launch; the epoch plan is the host dataset's own token order cut into the
batches ``batches()`` yields; the scheme driver refuses the key wherever the step cannot be resident."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import device_data_cases as DC
from egt_amd import data as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_struct_layout_and_abi_version(egt_lib, tmp_path):
    from egt_amd import _lib as L
    raw = C.CDLL(egt_lib._name)
    for sym in ("egt_batch_assemble_at", "egt_accumulate"):
        assert hasattr(raw, sym) and sym in L._PROTOS
    assert egt_lib.egt_abi_version() == 4 and L.ABI_VERSION == 4
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "egt_amd.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(egt_acc_item));']
    lines += [f'  printf("{f} %zu\\n", offsetof(egt_acc_item, {f}));' for f, _ in L.AccItem._fields_]
    lines += ['  printf("abi %d\\n", EGT_ABI_VERSION);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(ln.rsplit(" ", 1) for ln in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(L.AccItem) == 24
    for f, _ in L.AccItem._fields_:
        assert int(got[f]) == getattr(L.AccItem, f).offset, f
    assert int(got["abi"]) == 4


def _desc(L, **kw):
    d = dict(B=2, N=8, records=4, node_kind=L.BATCH_I32, node_width=1, edge_kind=L.BATCH_I32, edge_width=1, pe_kind=L.BATCH_PE_NONE,
             pe_features=0, target_kind=L.BATCH_TGT_GRAPH_F32, flags=L.BATCH_MARK_INVALID, matrix_pad=0.0, mask_f=-1.0, mask_i=-1)
    d.update(kw)
    return L.BatchDesc(**d)


def test_argument_checks_without_a_device(egt_lib):
    """every refusal is returned before a launch: the pointers below are never dereferenced"""
    from egt_amd import _lib as L
    lib, err = egt_lib, lambda: egt_lib.egt_last_error_string()
    st, ot = L.BatchStore(), L.BatchOut()
    at = lambda d, s, idx, cur, o: lib.egt_batch_assemble_at(None if d is None else C.byref(d), None if s is None else C.byref(s), idx, cur,
                                                             None if o is None else C.byref(o), None)
    assert at(None, st, 64, 64, ot) == L.EGT_E_NULL
    assert at(_desc(L, N=513), st, 64, 64, ot) == L.EGT_E_SHAPE                    # egt_batch_assemble's own coverage
    bad = _desc(L)
    bad.reserved[0] = 1
    assert at(bad, st, 64, 64, ot) == L.EGT_E_FLAGS and b"reserved" in err()        # reserved stays 0
    assert at(_desc(L), None, 64, 64, ot) == L.EGT_E_NULL
    assert at(_desc(L), st, None, 64, ot) == L.EGT_E_NULL and b"idx_table" in err()
    assert at(_desc(L), st, 64, None, ot) == L.EGT_E_NULL and b"cursor" in err()
    assert at(_desc(L), st, 64, 68, ot) == L.EGT_E_SHAPE and b"8-byte" in err()
    assert at(_desc(L), st, 64, 64, None) == L.EGT_E_NULL
    assert at(_desc(L), st, 64, 64, ot) == L.EGT_E_NULL and b"store.num_nodes" in err()
    # the plain entry gives the same answers for the same descriptor and store
    assert lib.egt_batch_assemble(C.byref(_desc(L)), C.byref(st), 64, C.byref(ot), None) == L.EGT_E_NULL and b"store.num_nodes" in err()
    acc = lib.egt_accumulate
    assert acc(None, 64, 3, None) == L.EGT_E_NULL and b"acc" in err()
    assert acc(64, None, 3, None) == L.EGT_E_NULL and b"items" in err()
    for K in (0, -1, 33, 1 << 20):
        assert acc(64, 64, K, None) == L.EGT_E_SHAPE and b"1..32" in err()
    assert acc(68, 64, 3, None) == L.EGT_E_SHAPE
    with pytest.raises(ValueError):
        from egt_amd.graph import DeviceAccumulator
        DeviceAccumulator(33, "cpu")


def _tokens_and_shapes(ds, split, batch_size, drop_remainder):
    """the host pipeline's own epoch: (tokens in order, [(B, N)]) of ``batches()``"""
    toks, shapes = [], []
    for b in ds.batches(split, batch_size, drop_remainder=drop_remainder, as_torch=False):
        toks += [t.decode() if isinstance(t, bytes) else str(t) for t in b["record_name"]]
        shapes.append(tuple(b["graph_matrix"].shape[:2]))
    return toks, shapes


@pytest.mark.parametrize("name,level,max_length", [("zinc", "matrix", None), ("sbm_pattern", "matrix", None), ("zinc", "matrix", 40)])
@pytest.mark.parametrize("drop_remainder", [False, True])
def test_epoch_plan_is_the_host_epoch(name, level, max_length, drop_remainder, tmp_path):
    """13 training graphs in batches of 4: three full batches and a last one of ONE graph (dropped under drop_remainder), over
    two epochs of the same generator (the second epoch continues the first one's draws)"""
    from egt_amd.device_data import pack_split, plan_epoch
    path = DC.edge_case_store(tmp_path, name)
    kw = dict(level=level, max_length=max_length, max_shuffle_len=6, seed=11, prefetch_batch=False)
    host, other = D.GraphDataset(name, path, **kw), D.GraphDataset(name, path, **kw)
    packed = pack_split(other, "training")
    index = {t: i for i, t in enumerate(packed["tokens"])}
    seen = []
    for epoch in range(2):
        toks, shapes = _tokens_and_shapes(host, "training", 4, drop_remainder)
        plan = plan_epoch(other, "training", index, packed["num_nodes"], 4, drop_remainder)
        assert [packed["tokens"][i] for i in plan.ids] == toks, epoch
        assert plan.batches == shapes and len(plan) == (3 if drop_remainder else 4), (epoch, plan.batches, shapes)
        assert plan.ids.dtype == np.int32 and plan.offsets.tolist() == [0, 4, 8, 12][:len(plan)]
        if not drop_remainder:
            assert plan.batches[-1][0] == 1
        seen.append(plan.ids.tolist())
    assert seen[0] != seen[1], "the second epoch is reshuffled"
    # the validation split is not shuffled: store order
    plan = plan_epoch(other, "validation", {t: i for i, t in enumerate(pack_split(other, "validation")["tokens"])},
                      pack_split(other, "validation")["num_nodes"], 2, False)
    assert plan.ids.tolist() == [0, 1, 2, 3, 4] and [b for b, _ in plan.batches] == [2, 2, 1]


def _scheme(cfg, device=None):
    from egt_amd import training as T
    return T.ZincSVDScheme(dict(dict(model_width=16, edge_width=16, model_height=1), **cfg), device=device, print_fn=lambda *a: None)


def test_the_key_exists_and_is_off_by_default():
    from egt_amd import training as T
    for scheme in T.SCHEMES:
        assert T.default_config(scheme).resident_step is False
    assert T.make_config(dict(resident_step=True)).resident_step is True


@pytest.mark.parametrize("have", [(), ("use_hipgraph",), ("fused_optimizer", "device_dataset"), ("use_hipgraph", "device_dataset")])
def test_refused_without_each_of_the_three_keys(have):
    keys = ("use_hipgraph", "fused_optimizer", "device_dataset")
    s = _scheme(dict(resident_step=True, **{k: True for k in have}))
    with pytest.raises(ValueError) as e:
        s._resident_check()
    for k in keys:
        assert (f"config.{k}" in str(e.value)) == (k not in have), (k, str(e.value))


def test_refused_off_the_gpu_and_with_more_than_one_rank(monkeypatch):
    from egt_amd import training as T
    on = dict(resident_step=True, use_hipgraph=True, fused_optimizer=True, device_dataset=True)
    for dev in (None, "cpu", torch.device("cpu")):
        with pytest.raises(ValueError, match="GPU"):
            _scheme(on, device=dev)._resident_check()
    with pytest.raises(ValueError):                                     # load_model refuses too (whichever key's check comes first)
        _scheme(on, device="cpu").load_model()
    s = _scheme(on, device="cuda")                                      # (nothing touches the device in the check)
    s._resident_check()
    monkeypatch.setattr(T, "_dist_on", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError, match="2 ranks"):
        s._resident_check()
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 1)
    s._resident_check()                                                 # an initialised group of one rank is one process
    _scheme(dict(on, resident_step=False), device="cpu")._resident_check()     # key off: nothing is asked


def test_train_step_needs_the_schemes_own_dataset():
    from egt_amd import training as T
    s = _scheme(dict(resident_step=True, use_hipgraph=True, fused_optimizer=True, device_dataset=True), device="cuda")
    s._resident, s.model = True, torch.nn.Linear(1, 1)
    with pytest.raises(ValueError, match="device-resident dataset"):
        s.train_step(dict(node_features=torch.zeros(1)))
    s._resident = False                                                 # (nothing captured: __del__ has nothing to wait for)
