"""The oracle, pinned by EXECUTING the reference's model code (oracle/ref_exec.py on the eager stand-in oracle/tf_eager).

  * regeneration      every fixture of tests/golden/reference/ is recomputed from the reference tree and equals the committed
                      file: inputs, weights, masks and distance target bit for bit, the fp64 outputs within 1e-12 of the
                      tensor's magnitude (summation order differs between torch builds and thread counts; bit equality of
                      fp64 sums would test the machine); the oracle is compared with the WHOLE reference tensors there
  * oracle vs fixture the same comparison against what the committed files hold -- runs without the reference tree
  * fp32 mode         the additive masks round to exactly -1e9: all-masked rows are uniform over their least-masked keys
  * the comparison can fail, the stand-in's Keras rules against hand-written values, and nothing leaks out of the context

The parts that need the reference tree (EGT_REFERENCE_DIR, default /root/reference) skip where it is absent.

Bound: |a - r| <= 1e-12 * max|r| per tensor, max over the WHOLE reference tensor (the fixture stores it).  Both sides are fp64
evaluations of the same formulas in different operation orders: measured worst 2.4e-15 (stacks), 1e-15 (blocks), 0 or 1 ulp
(inner op).  A tensor that is identically zero in exact arithmetic -- d dense_edge_b.bias where the bias only feeds the
softmax: a sum of softmax-row gradients -- is rounding noise (1e-17) on both sides and max|r| says nothing about it; as in
tests/util.py it is recognised by max|r| < 1e-9 and held to the absolute bound 1e-12, the relative bound at magnitude 1.
"""
import importlib
import math
import sys

import numpy as np
import pytest
import torch

import reference_cases as RC
from oracle import egt_oracle as O, ref_exec as RX
from oracle import tf_eager as tf
from util import assert_close, FWD

REL = 1e-12
needs_reference = pytest.mark.skipif(not RX.available(), reason="no reference tree (EGT_REFERENCE_DIR)")
CASE_IDS = [f"{f}-{n}" for f, n in RC.ALL_CASES]


@pytest.fixture
def ref():
    with RX.reference() as R:
        yield R


def _bound(maxabs):
    return REL * (maxabs if maxabs >= 1e-9 else 1.0)


def _check_values(name, a, r, maxabs):
    a, r = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(r, dtype=np.float64).reshape(-1)
    assert a.shape == r.shape, f"{name}: {a.shape} against {r.shape}"
    assert np.isfinite(a).all() and np.isfinite(r).all(), f"{name}: non-finite values"
    err = float(np.abs(a - r).max()) if a.size else 0.0
    assert err <= _bound(maxabs), f"{name}: |a - r| up to {err:.3e} > {_bound(maxabs):.3e} (max|r| {maxabs:.3e})"
    return err


def compare_with_fixture(family, name, fix=None):
    """the oracle's tensors against the reference's stored ones; -> the worst |a - r| / max|r|"""
    fix = fix or RC.load(family, name)
    out, bits = RC.oracle_case(family, name)
    assert set(out) == set(fix["stat"]), set(out) ^ set(fix["stat"])
    worst = 0.0
    for k, v in out.items():
        s, ss, mx = fix["stat"][k]
        err = _check_values(f"{family}_{name}: {k}", RC.picked(fix, k, v).numpy(), fix[f"out/{k}"], mx)
        worst = max(worst, err / (mx if mx >= 1e-9 else 1.0))
        whole = v.detach().double().reshape(-1)
        n = max(whole.numel(), 1)
        assert abs(float(whole.sum()) - s) <= n * _bound(mx), f"{family}_{name}: sum of {k}"
        assert abs(float((whole * whole).sum()) - ss) <= 2 * n * _bound(mx) * max(mx, 1.0), f"{family}_{name}: sum of squares of {k}"
    stored_bits = {k[5:] for k in fix["sha"] if k.startswith("bits/")}
    assert stored_bits == set(bits), stored_bits ^ set(bits)
    for k, v in bits.items():
        assert np.array_equal(RC.sha(v), fix["sha"][f"bits/{k}"]), f"{family}_{name}: {k} is not bit-equal"
    return worst


# ------------------------------------------------------------------------------------- oracle against fixture -----
@pytest.mark.parametrize("family,name", RC.ALL_CASES, ids=CASE_IDS)
def test_oracle_matches_the_committed_reference_result(family, name):
    compare_with_fixture(family, name)


def test_fixture_sizes():
    import os
    sizes = [os.path.getsize(os.path.join(RC.REF_DIR, f)) for f in os.listdir(RC.REF_DIR)]
    assert len(sizes) == len(RC.ALL_CASES)
    assert max(sizes) <= 650 * 1024 and sum(sizes) < 2 * 1024 * 1024, (max(sizes), sum(sizes))


# ----------------------------------------------------------------------------------------------- regeneration -----
@needs_reference
@pytest.mark.parametrize("family,name", RC.ALL_CASES, ids=CASE_IDS)
def test_regenerated_fixture_equals_the_committed_one(family, name, ref):
    case = RC.ref_case(ref, family, name)
    new, old = RC.pack(case, RC.CAP[family]), RC.load(family, name)
    new_sha = dict(zip(new["sha_names"].tolist(), new["sha"]))
    assert set(new_sha) == set(old["sha"])
    for k, d in new_sha.items():                                     # inputs, weights, masks, distance target: bit-equal
        assert np.array_equal(d, old["sha"][k]), f"{k} changed"
    for k in new["stat_names"].tolist():
        mx = old["stat"][k][2]
        # fp64 outputs: NOT array_equal.  The same code on another torch build or thread count sums in another order (matmul
        # blocking, reduction trees): last-bit differences that say nothing about the reference or the stand-in.  They are
        # held to the bound every comparison here uses; everything integer, boolean or fp32 above is bit-equal.
        _check_values(f"{k} (regenerated)", new[f"out/{k}"], old[f"out/{k}"], mx)
    # the oracle against the WHOLE tensors of the live reference run
    out, bits = RC.oracle_case(family, name)
    assert set(out) == set(case["out"])
    for k, v in out.items():
        r = case["out"][k].detach().as_subclass(torch.Tensor).double()
        assert tuple(v.shape) == tuple(r.shape), k
        _check_values(f"{k} (whole tensor)", v.detach().double().numpy(), r.numpy(), float(r.abs().max()) if r.numel() else 0.0)
    for k, v in bits.items():
        assert torch.equal(v.to(torch.int64), case["bits"][k].to(torch.int64)), k


# -------------------------------------------------------------------------------------------------- fp32 mode -----
def _allmasked_inputs(gated):
    g = torch.Generator().manual_seed(6)
    B, N, Hh, d = 1, 6, 8, 8
    QKV = torch.randn(B, N, 3 * d * Hh, generator=g)
    E = torch.randn(B, N, N, Hh, generator=g); G = torch.randn(B, N, N, Hh, generator=g) if gated else None
    mask = torch.zeros(B, N, dtype=torch.bool)                       # every key masked: -1e9
    M = torch.ones(B, N, N, Hh); M[:, :, 4:, :] = 0.0                # keys 4, 5 masked twice: -2e9
    return QKV, E, G, M, mask


@needs_reference
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
def test_fp32_all_masked_rows(gated, ref):
    QKV, E, G, M, mask = _allmasked_inputs(gated)

    def run(dtype, gate=gated):
        layer = ref.egt_layers.EGT(num_heads=8, gate_input=gate, attn_mask=True, name="mha")
        with RX.session(dtype=dtype):
            args = [RX.masked(QKV.to(dtype), mask), RX.wrap(E.to(dtype))] + ([RX.wrap(G.to(dtype))] if gate else []) + [RX.wrap(M.to(dtype))]
            return [t.as_subclass(torch.Tensor) for t in layer(args)]

    V32, H32, A32 = run(torch.float32)
    assert A32.dtype == torch.float32
    cv = lambda t: None if t is None else t.double()
    Vo, Ho, Ao = O.egt_forward(cv(QKV), cv(E), cv(G), cv(M), mask, num_heads=8)
    if gated:
        assert float(A32.abs().max()) == 0.0 and float(V32.abs().max()) == 0.0      # sigmoid(G - 1e9) is exactly 0
        # the gated layer returns softmax * gates only; its softmax row is what the reference's ungated layer computes from the
        # same logits (call_gated and call_ungated build H_hat_ line for line alike): exactly uniform over the least-masked keys
        S32 = run(torch.float32, gate=False)[2]
        assert torch.equal(S32[:, :, :4], torch.full_like(S32[:, :, :4], 0.25)) and float(S32[:, :, 4:].abs().max()) == 0.0
    else:
        assert torch.equal(A32[:, :, :4], torch.full_like(A32[:, :, :4], 0.25)), "not uniform over the least-masked keys"
        assert float(A32[:, :, 4:].abs().max()) == 0.0
        # evaluated in fp64 the same code keeps the logit differences: the row is not uniform.  This is why the fp64 oracle
        # reproduces the fp32 rounding of the masked sums (oracle/egt_oracle.py: _add_mask)
        A64 = run(torch.float64)[2]
        assert float((A64[:, :, :4] - 0.25).abs().max()) > 1e-3
    assert_close(A32, Ao, name="A_tild", **FWD)
    assert_close(V32, Vo, name="V_att", **FWD)
    assert_close(H32, Ho, name="H_hat", **FWD)


# ---------------------------------------------------------------------------------- the comparison can fail -----
def _wrong_forward(variant):
    """egt_layers.py:57-143 restated WRONG in one place (gated, key mask, no attention mask, nothing stochastic)"""
    def forward(QKV, E, G, M, mask, *, num_heads=8, clip_logits_value=(-5.0, 5.0), **kw):
        B, N, C = QKV.shape
        d = C // (3 * num_heads)
        Q, K, V = QKV.reshape(B, N, 3, d, num_heads).unbind(2)
        A = torch.einsum("bldh,bmdh->blmh", Q, K)
        if variant == "clip_before_scale":
            A = torch.clamp(A, *clip_logits_value) * d ** -0.5
        else:
            A = torch.clamp(A * d ** -0.5, *clip_logits_value)
        Hh = A + E
        m_ = (mask[:, None, :, None].to(QKV.dtype) - 1) * 1e9
        S = torch.softmax(O._add_mask(Hh, m_), dim=2)
        gates = torch.sigmoid(G) if variant == "gate_before_mask" else torch.sigmoid(O._add_mask(G, m_))
        At = S * gates
        return torch.einsum("blmh,bmdh->bldh", At, V).reshape(B, N, d * num_heads), Hh, At
    return forward


def test_the_unbroken_stand_ins_of_the_wrong_restatements_pass(monkeypatch):
    """the scaffold of _wrong_forward with no mistake in it passes: the three failures below are due to the mistakes"""
    monkeypatch.setattr(O, "egt_forward", _wrong_forward(None))
    compare_with_fixture("attn", "gated_d8_clip")
    compare_with_fixture("attn", "gated_allmasked")


@pytest.mark.parametrize("variant,family,name", [("clip_before_scale", "attn", "gated_d8_clip"),
                                                 ("gate_before_mask", "attn", "gated_allmasked"),
                                                 ("edge_r_reads_a_tild", "block", "residual_zinc500k")])
def test_a_wrong_restatement_is_caught(variant, family, name, monkeypatch):
    if variant == "edge_r_reads_a_tild":
        good = O.egt_forward
        monkeypatch.setattr(O, "egt_forward", lambda *a, **k: (lambda V, Hh, At: (V, At, At))(*good(*a, **k)))
    else:
        monkeypatch.setattr(O, "egt_forward", _wrong_forward(variant))
    with pytest.raises(AssertionError, match=r"\|a - r\| up to"):
        compare_with_fixture(family, name)


# ------------------------------------------------------------------------------------- stand-in self-checks -----
L = tf.keras.layers


def _t(v, dtype=torch.float64):
    return RX.wrap(torch.tensor(v, dtype=dtype))


def test_standin_mask_propagation():
    with RX.session(weights={"d/kernel": [[1.0], [1.0]], "d/bias": [0.0]}):
        x = RX.masked(_t([[[1.0, 2.0], [3.0, 4.0]]]), torch.tensor([[True, False]]))
        y = L.Dense(1, name="d")(x)
        assert y.tolist() == [[[3.0], [7.0]]]
        assert y._keras_mask.tolist() == [[True, False]]                          # Dense passes the mask on
        assert L.Lambda(lambda v: v * 2, name="l")(y)._keras_mask is None         # a Lambda without mask= drops it
        z = L.Lambda(lambda v, mask: v * 2, mask=lambda i, m: ~m, name="l2")(y)   # with mask=: computes it
        assert z._keras_mask.tolist() == [[False, True]]
        other = RX.masked(_t([[[1.0], [1.0]]]), torch.tensor([[False, False]]))
        nomask = _t([[[1.0], [1.0]]])
        assert L.Add(name="a")([y, nomask])._keras_mask.tolist() == [[True, False]]     # None masks do not count
        assert L.Add(name="b")([y, other])._keras_mask.tolist() == [[False, False]]     # AND of the others
        assert L.Add(name="c")([nomask, nomask])._keras_mask is None
        assert L.Flatten(name="f")(y)._keras_mask is None                         # no masking support: dropped
        assert y.shape.rank == 3 and tf.shape(y)[2] == 1
        y.set_shape([None, 2, 1])
        with pytest.raises(ValueError):
            y.set_shape([None, 3, 1])


def test_standin_list_inputs_get_one_mask_each():
    seen = {}

    class Probe(L.Layer):
        def call(self, inputs, mask=None, training=None):
            seen.update(mask=mask, training=training)
            return inputs[0] + 0

        def compute_mask(self, inputs, mask=None):
            return None

    a = RX.masked(_t([1.0]), torch.tensor([True])); b = _t([2.0])
    with RX.session(training=True):
        Probe(name="p")([a, b])
        assert seen["mask"][0].tolist() == [True] and seen["mask"][1] is None and seen["training"] is True
        Probe(name="q")([b, b])
        assert seen["mask"] is None                                               # all None: no list of Nones


def test_standin_embedding_mask_zero():
    table = [[10.0, 11.0], [20.0, 21.0], [30.0, 31.0]]
    with RX.session(weights={"emb/embeddings": table}):
        y = L.Embedding(3, 2, mask_zero=True, name="emb")(_t([[0.0, 2.0, 1.0]]))
    assert y.tolist() == [[[10.0, 11.0], [30.0, 31.0], [20.0, 21.0]]]              # row 0 is an ordinary row
    assert y._keras_mask.tolist() == [[False, True, True]]


def test_standin_masking_layer_and_masked_pooling():
    with RX.session():
        x = L.Masking(mask_value=-1.0, name="m")(_t([[[-1.0, -1.0], [-1.0, 2.0], [3.0, 4.0]]]))
        assert x.tolist() == [[[0.0, 0.0], [-1.0, 2.0], [3.0, 4.0]]] and x._keras_mask.tolist() == [[False, True, True]]
        pooled = L.GlobalAveragePooling1D(name="p")(x)
        assert pooled.tolist() == [[1.0, 3.0]] and getattr(pooled, "_keras_mask", None) is None
        assert L.GlobalAveragePooling1D(name="p2")(_t([[[0.0, 0.0], [-1.0, 2.0], [4.0, 4.0]]])).tolist() == [[1.0, 2.0]]


def test_standin_inverted_dropout_and_injection():
    x = _t([1.0, 2.0, 3.0, 4.0])
    with RX.session(training=True, keep_by_name={"drop": torch.tensor([1, 0, 1, 1])}, keep=[torch.tensor([0, 1, 1, 1])]):
        assert L.Dropout(0.2, name="drop")(x).tolist() == [1.25, 0.0, 3.75, 5.0]
        assert tf.nn.dropout(x, 0.5).tolist() == [0.0, 4.0, 6.0, 8.0]
    with RX.session(training=False):
        assert L.Dropout(0.2, name="drop")(x).tolist() == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(RuntimeError, match="no injected"):
        with RX.session(training=True):
            L.Dropout(0.2, name="drop")(x)
    with pytest.raises(RuntimeError, match="never asked for"):
        with RX.session(uniform=[torch.zeros(2)]):
            pass
    with RX.session(uniform=[torch.tensor([0.0, 1.0])]):
        assert tf.where(tf.random.uniform([2], minval=0., maxval=1.) < 0.3, -1e9, 0.).tolist() == [-1e9, 0.0]


def test_standin_layer_norm_epsilon_and_unloaded_weights():
    with RX.session(weights={"ln/gamma": [2.0, 2.0], "ln/beta": [0.5, 0.5]}):
        y = L.LayerNormalization(name="ln")(_t([[1.0, 3.0]]))                     # mean 2, biased variance 1, epsilon 1e-3
    r = 1.0 / math.sqrt(1.0 + 1e-3)
    assert y.tolist()[0] == pytest.approx([-2.0 * r + 0.5, 2.0 * r + 0.5], rel=1e-15)
    assert abs(y.tolist()[0][1] - 2.5) > 5e-4                                     # epsilon 1e-3, not 1e-6 or 0
    with RX.session():
        assert torch.isnan(L.Dense(1, name="nobody_loads_me")(_t([[1.0]]))).all()
    with pytest.raises(KeyError):
        with RX.session(weights={"x/kernel": [[1.0]]}):
            L.Dense(1, name="x")(_t([[1.0]]))                                     # x/bias was not given


def test_standin_dtype_modes_and_small_functions():
    with RX.session(dtype=torch.float32):
        m = (tf.cast(_t([True, False], torch.bool), tf.float32) - 1) * 1e9
        assert m.dtype == torch.float32 and (_t([3.5, 0.0], torch.float32) + m).tolist() == [3.5, -1e9]   # rounds to -1e9
    with RX.session():
        assert tf.cast(_t([True], torch.bool), tf.float32).dtype == torch.float64                        # the working dtype
        assert tf.math.round(_t([0.5, 1.5, 2.5])).tolist() == [0.0, 2.0, 2.0]
        assert tf.math.divide_no_nan(_t([1.0, 2.0]), _t([0.0, 4.0])).tolist() == [0.0, 0.5]
        assert tf.pad(_t([[1.0]]), [(1, 0), (0, 2)], constant_values=9).tolist() == [[9.0, 9.0, 9.0], [1.0, 9.0, 9.0]]
        assert tf.one_hot(_t([2, 0], torch.int64), 3).tolist() == [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]
        x = _t([-7.0, 0.0, 7.0]).requires_grad_()
        tf.clip_by_value(x, -5., 5.).sum().backward()
        assert x.grad.tolist() == [0.0, 1.0, 0.0]
        ce = tf.keras.backend.sparse_categorical_crossentropy(_t([1], torch.int64), _t([[0.0, 0.0]]), from_logits=True)
        assert ce.tolist() == pytest.approx([math.log(2.0)], rel=1e-15)


# ------------------------------------------------------------------------------------------------- leak check -----
def _import_error(name):
    try:
        importlib.import_module(name)
    except ImportError as ex:
        return type(ex).__name__
    return None


@needs_reference
def test_nothing_leaks_out_of_the_context():
    before, path_before = _import_error("tensorflow"), list(sys.path)
    assert "lib" not in sys.modules
    with RX.reference() as R:
        import tensorflow
        assert tensorflow is tf and R.egt_layers.__name__ == "lib.models.egt_layers"
        assert sys.modules["tensorflow.keras.layers"] is tf.keras.layers
    assert not [n for n in sys.modules if n == "lib" or n.startswith(("lib.", "tensorflow"))]
    assert sys.path == path_before
    assert _import_error("tensorflow") == before
    if before is not None:
        with pytest.raises(ImportError):
            import tensorflow  # noqa: F401,F811


def test_reference_context_refuses_an_absent_tree(monkeypatch, tmp_path):
    monkeypatch.setenv("EGT_REFERENCE_DIR", str(tmp_path))
    assert not RX.available()
    with pytest.raises(FileNotFoundError):
        with RX.reference():
            pass
    assert "tensorflow" not in sys.modules


def test_weight_helpers_round_trip():
    with RX.session():
        d = L.Dense(2, name="dense_qkv_00")
        d(_t([[1.0, 2.0, 3.0]]))
    tracked = {"dense_qkv_00": d}
    assert list(RX.named_weights(tracked)) == ["dense_qkv_00/kernel", "dense_qkv_00/bias"]
    vals = {"dense_qkv_00/kernel": np.arange(6.0).reshape(3, 2), "dense_qkv_00/bias": np.array([1.0, -1.0])}
    RX.load_weights(tracked, vals)
    back = RX.read_weights(tracked)
    assert all(np.array_equal(back[k].numpy(), v) for k, v in vals.items())
    with RX.session():
        y = d(_t([[1.0, 1.0, 1.0]]))
    assert y.tolist() == [[7.0, 8.0]]
    g = RX.weight_grads(tracked, y.sum())
    assert g["dense_qkv_00/kernel"].tolist() == [[1.0, 1.0]] * 3 and g["dense_qkv_00/bias"].tolist() == [1.0, 1.0]
    with pytest.raises(KeyError):
        RX.load_weights(tracked, {"dense_qkv_00/kernel": vals["dense_qkv_00/kernel"]})
    assert RC.keras_name("layer3.ffn_edge.lr1_kernel") == "fnn_lr1_edge_03/kernel"
    assert RC.keras_name("layer0.ffn_node.norm_beta") == "norm_fnn_node_00/beta"
    assert RC.keras_name("layer12.dense_qkv.bias") == "dense_qkv_12/bias" and RC.keras_name("adj_emb.kernel") == "adj_emb/kernel"
