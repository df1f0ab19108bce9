"""Memory-contract harness for the C-ABI (include/egt_amd.h, "Buffer contract"): guarded buffers and a runner that executes
one call sequence with differently prefilled outputs / scratch.  No test functions here: tests/test_memcontract_cpu.py checks
the harness itself and the case table, tests/test_memcontract_gpu.py runs the entry points.

Arena: one uint8 tensor laid out as [guard | payload | guard].  The payload starts at a 512-byte-aligned address (what torch's
allocator gives every tensor) and has EXACTLY the byte count the header / the size query states; each guard is at least one
graph's slice of the buffer (ceil(bytes / B) rounded up to 512) and at least 4 KiB, so a write that is off by one row, tile,
partial slot or graph lands in memory the test owns.  Guards hold a seeded pseudo-random byte pattern.

A shifted arena (`shift` bytes, a multiple of the element size) starts its payload that many bytes past the 512-aligned address:
same byte count, guards still directly adjacent on both sides (the leading one grows by `shift`).  That is how a parameter
tensor or a gradient sink reaches the C ABI from one flat buffer: aligned to its element and to nothing more.

Runner: every tensor of a case lives in an arena (inputs and parameters too).
  run Z   outputs, carried buffers and scratch prefilled with 0x00
  run P   ... with 0xFF (NaN as fp32 and bf16, 255 as uint8); carried buffers (forward -> backward) are poisoned before the
          first step only, plain scratch again before every step
  run A   one run per aliasing the header allows (Z prefill)
  run U-* cases with buffers of a pointer class (PARAM: filled from an nn.Parameter, SINK: from its .grad) only; P prefill.
          The i-th such buffer of the case, in table order, is shifted by 4 (1 + i mod 3) bytes where the run shifts it:
          U-sinks  the SINK buffers (the layout FlatGradAllReduce(direct=True) produces)
          U-all    PARAM and SINK buffers
          U-mixed  half of each class -- its j-th buffer when j mod 4 is 0 or 3 -- so that one call sees aligned and
                   unaligned pointers together, neighbours of both kinds (dense_qkv.kernel and dense_mha.kernel, which
                   the node kernels test separately, land on different sides in every row of the tables)
and check(): guards bit-identical after every step, const inputs bit-identical to their snapshot, runs P and U-* finite,
Z == P, Z == A and Z == U-* bit for bit (alignment changes how operands reach LDS and registers, never the order of the
arithmetic)."""
from __future__ import annotations

import zlib

import torch

ALIGN = 512
GUARD_MIN = 4096
ZERO, POISON = 0x00, 0xFF
_ITYPE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _rup(x, a):
    return (x + a - 1) // a * a


def guard_bytes(nbytes, graphs=1):
    return max(GUARD_MIN, _rup(-(-nbytes // max(1, graphs)), ALIGN))


class GuardError(AssertionError):
    pass


class Arena:
    def __init__(self, name, nbytes, device="cpu", graphs=1, seed=0, shift=0):
        assert 0 <= shift < ALIGN
        self.name, self.nbytes, self.shift = name, int(nbytes), int(shift)
        g = self.g = guard_bytes(self.nbytes, graphs)
        raw = torch.empty(2 * g + shift + self.nbytes + ALIGN, dtype=torch.uint8, device=device)
        skip = (-raw.data_ptr()) % ALIGN            # 0 for torch's device allocations; host memory is only 64-byte aligned
        self.buf = raw[skip:skip + 2 * g + shift + self.nbytes]
        self.offset = g + shift                     # of the payload inside buf: the leading guard grows by the shift
        gen = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ seed) & 0x7FFFFFFF)
        pat = torch.randint(0, 256, (2 * g + shift,), generator=gen, dtype=torch.uint8).to(device)
        self._ref = (pat[:self.offset].clone(), pat[self.offset:].clone())
        self.before.copy_(self._ref[0])
        self.after.copy_(self._ref[1])

    @property
    def before(self):
        return self.buf[:self.offset]

    @property
    def after(self):
        return self.buf[self.offset + self.nbytes:]

    @property
    def payload(self):
        return self.buf[self.offset:self.offset + self.nbytes]

    def view(self, dtype, shape):
        return self.payload.view(dtype).view(*shape)

    def guard_faults(self):
        """[(side, first, last)]: byte offsets of the changed range, `before` counted back from the payload's first byte
        (1 = the byte just before it), `after` counted from the first byte past the payload (0 = that byte)."""
        out = []
        for side, cur, ref in (("before", self.before, self._ref[0]), ("after", self.after, self._ref[1])):
            if not torch.equal(cur, ref):
                idx = (cur != ref).nonzero().flatten()
                lo, hi = int(idx[0]), int(idx[-1])
                out.append((side, self.offset - hi, self.offset - lo) if side == "before" else (side, lo, hi))
        return out

    def check(self, when=""):
        for side, first, last in self.guard_faults():
            raise GuardError(f"buffer '{self.name}' ({self.nbytes} bytes): guard {side} the payload was written{when}: "
                             f"bytes {first}..{last} {'before its start' if side == 'before' else 'past its end'}")


# ---------------------------------------------------------------------------------------------------------- cases -----
IN, OUT, CARRIED, SCRATCH, INOUT = "in", "out", "carried", "scratch", "inout"
PARAM, SINK = "param", "sink"           # pointer classes: held to element alignment (4 bytes), not to torch's 512


class Buf:
    """One buffer of a case.
    role    IN       const input / parameter: `init` (a host tensor) gives dtype, shape and contents
            OUT      output or gradient sink (dtype, shape): compared between runs, finite in run P
            CARRIED  travels from the forward to the backward (saved, shared workspaces, rowstats, hops): prefilled once
            SCRATCH  plain workspace: prefilled before every step
            INOUT    read-modify-write argument (`init`): not const, compared between runs
    graphs  B, for the guard size
    ptr     PARAM (the Python side fills it from an nn.Parameter), SINK (from its .grad) or None (activations, masks, targets,
            seeds, saved buffers, workspaces: the 512-byte contract)
    exempt  (header sentence, mask_fn or None): elements excluded from "finite in P" and "Z == P" (mask_fn(view) -> bool tensor of
            the excluded elements; None = the whole buffer)
    compare CARRIED buffers only: also an output of the contract (rowstats)
    const_after   CARRIED: index of the step after which the header declares it const (bit-identical from then on), or None
    rmw     {step index: (header sentence, mask_fn)}: the documented read-modify-write exceptions to `const`"""

    def __init__(self, name, role, init=None, dtype=None, shape=None, nbytes=None, graphs=1, exempt=None, compare=None,
                 const_after=None, rmw=None, ptr=None):
        assert ptr is None or (ptr, role) in ((PARAM, IN), (SINK, OUT))
        self.name, self.role, self.init, self.graphs, self.ptr = name, role, init, graphs, ptr
        if init is not None:
            init = init.contiguous()
            self.init, dtype, shape = init, init.dtype, tuple(init.shape)
        if nbytes is not None and dtype is None:
            dtype, shape = torch.uint8, (int(nbytes),)
        self.dtype, self.shape = dtype, tuple(shape)
        n = 1
        for s in self.shape:
            n *= s
        self.esize = torch.empty((), dtype=dtype).element_size()
        self.nbytes = n * self.esize
        self.exempt, self.const_after, self.rmw = exempt, const_after, rmw or {}
        self.compare = (role in (OUT, INOUT)) if compare is None else compare


class Case:
    """name; bufs; steps: [fn(v)] with v = {buffer name: typed payload view} (each one C-ABI call, returns its status code);
    aliases: [{output buffer: the buffer whose memory it shares}] -- one run A each; claims: anything the CPU table test holds
    the case to (launch forms, size queries)."""

    def __init__(self, name, bufs, steps, aliases=(), **claims):
        self.name, self.bufs, self.steps, self.aliases, self.claims = name, list(bufs), list(steps), list(aliases), claims
        names = [b.name for b in self.bufs]
        assert len(set(names)) == len(names), f"{name}: duplicate buffer names"


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8)


U_RUNS = ("sinks", "all", "mixed")


def tagged(case):
    return [b for b in case.bufs if b.ptr is not None]


def shifts(case, which):
    """{buffer name: bytes} of run U-`which` (see the module's docstring)"""
    out, seen = {}, {PARAM: 0, SINK: 0}
    for i, b in enumerate(tagged(case)):
        j, seen[b.ptr] = seen[b.ptr], seen[b.ptr] + 1
        if {"sinks": b.ptr == SINK, "all": True, "mixed": j % 4 in (0, 3)}[which]:
            out[b.name] = 4 * (1 + i % 3)
            assert out[b.name] % b.esize == 0
    return out


def run(case, fill, device, alias=None, sync=None, check_rc=None, shift=None):
    """Execute the case's steps once.  Returns {name: clone of the typed payload} of every compared buffer."""
    alias, shift = alias or {}, shift or {}
    arenas, views = {}, {}
    for b in case.bufs:
        a = arenas[b.name] = Arena(f"{case.name}:{b.name}", b.nbytes, device, b.graphs, shift=shift.get(b.name, 0))
        if b.init is not None:
            a.payload.copy_(_bytes(b.init).to(device))
        else:
            a.payload.fill_(fill)
        views[b.name] = a.view(b.dtype, b.shape)
    by = {b.name: b for b in case.bufs}
    for dst, src in alias.items():
        assert by[dst].nbytes == by[src].nbytes
        views[dst] = arenas[src].view(by[dst].dtype, by[dst].shape)
    shared = set(alias.values())
    snap = {b.name: arenas[b.name].payload.clone() for b in case.bufs if b.role == IN and b.name not in shared}
    for i, step in enumerate(case.steps):
        if i:
            for b in case.bufs:
                if b.role == SCRATCH:
                    arenas[b.name].payload.fill_(fill)
        rc = step(views)
        if check_rc is not None:
            check_rc(rc)
        if sync is not None:
            sync()
        when = (f" by step {i} of case '{case.name}' (prefill 0x{fill:02X}{', aliased ' + str(alias) if alias else ''}"
                f"{', shifted ' + str(shift) if shift else ''})")
        for a in arenas.values():
            a.check(when)
        for name, s in list(snap.items()):
            cur, b = arenas[name].payload, by[name]
            if torch.equal(cur, s):
                continue
            bad = arenas[name].view(b.dtype, b.shape).view(_ITYPE[b.esize]) != s.view(b.dtype).view(*b.shape).view(_ITYPE[b.esize])
            if i in b.rmw:                      # a documented read-modify-write: only those elements may change
                bad &= ~b.rmw[i][1](views[name]).expand(b.shape)
                snap[name] = cur.clone()
            if bad.any():
                idx = bad.flatten().nonzero().flatten()
                raise AssertionError(f"const buffer '{case.name}:{name}' was written{when}: {int(bad.sum())} elements, "
                                     f"flat indices {int(idx[0])}..{int(idx[-1])}, shape {b.shape}")
        for b in case.bufs:
            if b.role == CARRIED and b.const_after == i and b.name not in shared:
                snap[b.name] = arenas[b.name].payload.clone()
    return {b.name: views[b.name].clone() for b in case.bufs if b.compare}


def _excluded(b, t):
    if b.exempt is None:
        return None
    fn = b.exempt[1]
    return torch.ones(t.shape, dtype=torch.bool, device=t.device) if fn is None else fn(t).expand(t.shape)


def assert_finite(case, outs, run_name="P"):
    for b in case.bufs:
        if not b.compare or not b.dtype.is_floating_point:
            continue
        t = outs[b.name]
        bad = ~torch.isfinite(t.float())
        ex = _excluded(b, t)
        if ex is not None:
            bad &= ~ex
        if bad.any():
            idx = bad.flatten().nonzero().flatten()
            raise AssertionError(f"'{case.name}:{b.name}' run {run_name}: {int(bad.sum())}/{t.numel()} elements are not finite "
                                 f"(the prefill shows through: never written, or computed from an unwritten word); flat "
                                 f"indices {int(idx[0])}..{int(idx[-1])}, shape {tuple(t.shape)}")


def assert_same_bits(case, ref, got, names=("Z", "P")):
    for b in case.bufs:
        if not b.compare:
            continue
        r, g = ref[b.name], got[b.name]
        itype = _ITYPE[r.element_size()]
        bad = r.view(itype) != g.view(itype)
        ex = _excluded(b, r)
        if ex is not None:
            bad &= ~ex
        if bad.any():
            idx = bad.flatten().nonzero().flatten()
            raise AssertionError(f"'{case.name}:{b.name}': run {names[1]} differs from run {names[0]} in {int(bad.sum())}/{r.numel()} "
                                 f"elements, flat indices {int(idx[0])}..{int(idx[-1])}, shape {tuple(r.shape)} "
                                 f"(first: {r.flatten()[idx[0]].item()!r} vs {g.flatten()[idx[0]].item()!r})")


def check(case, device, sync=None, check_rc=None, u_runs=U_RUNS):
    """Runs Z, P, every A and (where the case has buffers of a pointer class) the U runs of the case and asserts the contract;
    returns run Z's outputs (for the oracle / wrapper checks)."""
    z = run(case, ZERO, device, sync=sync, check_rc=check_rc)
    p = run(case, POISON, device, sync=sync, check_rc=check_rc)
    assert_finite(case, p)
    assert_same_bits(case, z, p)
    for al in case.aliases:
        a = run(case, ZERO, device, alias=al, sync=sync, check_rc=check_rc)
        assert_same_bits(case, z, a, names=("Z", f"A {al}"))
    for which in (u_runs if tagged(case) else ()):
        u = run(case, POISON, device, sync=sync, check_rc=check_rc, shift=shifts(case, which))
        assert_same_bits(case, z, u, names=("Z", f"U-{which}"))
        assert_finite(case, u, f"U-{which}")
    return z


# ============================================================================================ the case table ==========
# Builders of the cases both test files use.  They only need the loaded library for its size queries (which answer
# without a GPU); inputs are host tensors, copied into the arenas of the run's device.
import ctypes as C  # noqa: E402

BLOCK_ORACLE_NAMES = ("norm_edge.gamma", "norm_edge.beta", "attention_gates.kernel", "attention_gates.bias",
                      "dense_edge_b.kernel", "dense_edge_b.bias", "norm_mha.gamma", "norm_mha.beta", "dense_qkv.kernel",
                      "dense_qkv.bias", "dense_mha.kernel", "dense_mha.bias", "dense_edge_r.kernel", "dense_edge_r.bias")
STATIC_NULL = (0, 1, 12, 13)          # EGT_BF_STATIC_EDGE: norm_edge_* / dense_edge_r_* "are never read and may be NULL"
RAND_P, SEED, STACK_LAYERS = 0.25, 0x5EED1234ABCD, 3

# (id, B, N, d, De, bf16, extras, forward form, backward form) -- the forms are what egt_block_launch_form answers in a process
# without plan switches; tests/test_memcontract_cpu.py holds the table to them.
BLOCK_TABLE = [
    ("n19_de8", 2, 19, 8, 8, False, "", "k_narrow_fwd/4w", "k_narrow_bwd/4w/tl8"),
    ("n37_de8_bf16", 2, 37, 8, 8, True, "", "k_narrow_fwd/4w", "k_narrow_bwd/4w/tl8"),
    ("n70_de8", 1, 70, 8, 8, False, "", "k_narrow_fwd/8w/half", "k_narrow_bwd/8w/tl8"),
    ("n70_de8_b26", 26, 70, 8, 8, False, "", "k_narrow_fwd/8w", "k_narrow_bwd/8w/tl8"),      # 8 waves, 16-row workgroups
    ("n19_de8_static", 2, 19, 8, 8, False, "static", "k_narrow_fwd/4w", "k_narrow_bwd/4w/tl8"),
    ("n19_de8_static_null_deo", 2, 19, 8, 8, False, "static,null_deo", "k_narrow_fwd/4w", "k_narrow_bwd/4w/tl8"),
    ("n21_de16", 2, 21, 8, 16, False, "", "k_block_fwd_r4/4w", "k_block_bwd_v4r/4w/tl4"),
    ("n150_de16", 1, 150, 8, 16, False, "", "k_block_fwd_r4/8w", "k_block_bwd_v4r/4w/tl4"),
    ("n300_de16", 1, 300, 8, 16, False, "", "k_block_fwd/4w", "k_block_bwd_v4r/4w/tl4"),      # K/V do not fit in LDS
    ("n37_d6_de48", 3, 37, 6, 48, False, "", "k_block_fwd/4w", "k_block_bwd_v5/4w/tl4"),
    ("n19_de64", 2, 19, 8, 64, False, "", "k_block_fwd/4w", "k_block_bwd_v5/4w/tl4"),
    ("n33_de64_bf16", 2, 33, 8, 64, True, "", "k_block_fwd/4w", "k_block_bwd_v4/4w/tl4"),
    ("n21_de32_mask", 2, 21, 8, 32, False, "attn_mask", "k_block_fwd/4w", "k_block_bwd_v4/4w/tl4"),
    ("n19_de64_randmask", 2, 19, 8, 64, False, "rand_mask", "k_block_fwd/4w", "k_block_bwd_v5/4w/tl4"),
]
STACK_TABLE = [
    ("stack_n19_de64", 2, 19, 8, 64, False, "", "k_block_fwd/4w", "k_block_bwd_v5/4w/tl4"),
    ("stack_n37_de8_bf16", 2, 37, 8, 8, True, "", "k_narrow_fwd/4w", "k_narrow_bwd/4w/tl8"),
    ("stack_n21_de16", 2, 21, 8, 16, False, "", "k_block_fwd_r4/4w", "k_block_bwd_v4r/4w/tl4"),
    ("stack_n37_d6_de48", 3, 37, 6, 48, False, "", "k_block_fwd/4w", "k_block_bwd_v5/4w/tl4"),
]
# (row, layers): two shapes of tests/stack_tail.py's table (the 128-graph row: 27 five-step weight-gradient chunks and 384 edge
# partials per layer; the C ABI's 64-layer limit: six-step chunks, 176 partials, 6 + 4 closing launches) -- the backward tail's
# partial slots in the guarded workspace.  Run by tests/test_stack_tail_gpu.py (runs Z and P); stack_cases() keeps STACK_TABLE.
STACK_TAIL_TABLE = [
    (("tail_b128_n33_de8_ly16", 128, 33, 8, 8, False, "", "k_narrow_fwd/4w", "k_narrow_bwd/4w/tl11"), 16),
    (("tail_b44_n30_de16_ly64", 44, 30, 8, 16, False, "", "k_block_fwd_r4/4w", "k_block_bwd_v4r/4w/tl8"), 64),
]
# what the union of the two tables must reach (the issue's list)
REQUIRED_FORMS = {"fwd": {"k_narrow_fwd/4w", "k_narrow_fwd/8w", "k_narrow_fwd/8w/half", "k_block_fwd_r4/4w", "k_block_fwd_r4/8w",
                          "k_block_fwd"},
                  "bwd": {"k_narrow_bwd/4w", "k_narrow_bwd/8w", "k_block_bwd_v4r", "k_block_bwd_v5", "k_block_bwd_v4"}}


def _L():
    from egt_amd import _lib as L
    return L


def _stream():
    return _L().current_stream()


def _ptr(v, name):
    t = v.get(name)
    return None if t is None else C.c_void_p(t.data_ptr())


def _struct(cls, fields, v, prefix):
    return _L().params_struct(cls, fields, [v.get(prefix + f) for f in fields])


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _key_mask(B, N, tail):
    """every graph full but the last, whose `tail` last nodes are padding"""
    km = torch.ones(B, N, dtype=torch.uint8)
    if tail:
        km[B - 1, N - tail:] = 0
    return km


def block_desc(row):
    L = _L()
    _, B, N, d, De, bf16, extras, _, _ = row
    flags = L.BF_GATE | L.BF_CLIP | L.BF_TRAINING
    if "static" in extras:
        flags |= L.BF_STATIC_EDGE | L.BF_NO_EDGE_LN
    if "attn_mask" in extras:
        flags |= L.BF_ATTN_MASK
    return L.BlockDesc(B=B, N=N, H=8, d=d, De=De, dtype=L.EGT_BF16 if bf16 else L.EGT_F32, flags=flags, clip_lo=-5.0, clip_hi=5.0,
                       random_mask_prob=RAND_P, ln_eps=1e-3, reserved=0, seed=SEED, seed_device=None)


def block_inputs(row, layers=1):
    """host tensors of a block / stack case: dict(h, e, key_mask, attn_mask, rand_mask, dh, de, params: [layers][14])"""
    from oracle import egt_oracle as O
    name, B, N, d, De, bf16, extras, _, _ = row
    g = _gen(name)
    Dh, edt = 8 * d, (torch.bfloat16 if bf16 else torch.float32)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    inp = dict(h=r(B, N, Dh), e=(r(B, N, N, De) * 1.3 + 0.2).to(edt), key_mask=_key_mask(B, N, max(1, N // 6)),
               dh=r(B, N, Dh), de=r(B, N, N, De).to(edt), attn_mask=None, rand_mask=None)
    if "attn_mask" in extras:
        adj = (torch.rand(B, N, N, generator=g) > 0.5).to(torch.float32)
        inp["attn_mask"] = O.constrained_edge_mask(adj, 8).contiguous().float()
    if "rand_mask" in extras:
        inp["rand_mask"] = (torch.rand(B, N, N, 8, generator=g) < RAND_P).to(torch.uint8)
    inp["params"] = []
    for _ in range(layers):
        p = O.init_block_params(Dh, De, 8, dtype=torch.float32, generator=g, randomize_norm=True)
        inp["params"].append([p[k] for k in BLOCK_ORACLE_NAMES])
    return inp


def _block_bufs(row, inp, layers, saved_bytes, ws_bytes):
    L = _L()
    _, B, N, d, De, bf16, extras, _, _ = row
    static, null_deo = "static" in extras, "null_deo" in extras
    edt = torch.bfloat16 if bf16 else torch.float32
    bufs = [Buf("h", IN, inp["h"], graphs=B), Buf("e", IN, inp["e"], graphs=B), Buf("key_mask", IN, inp["key_mask"], graphs=B),
            Buf("d_h_out", IN, inp["dh"], graphs=B)]
    if not null_deo:
        bufs.append(Buf("d_e_out", IN, inp["de"], graphs=B))
    for k in ("attn_mask", "rand_mask"):
        if inp[k] is not None:
            bufs.append(Buf(k, IN, inp[k], graphs=B))
    for l in range(layers):
        for i, f in enumerate(L.BLOCK_PARAM_FIELDS):
            if static and i in STATIC_NULL:
                continue
            t = inp["params"][l][i]
            bufs.append(Buf(f"p{l}.{f}", IN, t, ptr=PARAM))
            bufs.append(Buf(f"g{l}.{f}", OUT, dtype=torch.float32, shape=t.shape, ptr=SINK))
    bufs += [Buf("h_out", OUT, dtype=torch.float32, shape=inp["h"].shape, graphs=B),
             Buf("d_h", OUT, dtype=torch.float32, shape=inp["h"].shape, graphs=B),
             Buf("d_e", OUT, dtype=edt, shape=inp["e"].shape, graphs=B),
             Buf("saved", CARRIED, nbytes=saved_bytes, graphs=B, const_after=0),
             Buf("ws", SCRATCH, nbytes=ws_bytes, graphs=B)]
    if static:      # "Forward: e_out is never written": handed over as a const buffer, so the runner holds it to its snapshot
        bufs.append(Buf("e_out", IN, torch.full(inp["e"].shape, 123.0).to(edt), graphs=B))
    else:
        bufs.append(Buf("e_out", OUT, dtype=edt, shape=inp["e"].shape, graphs=B))
    return bufs


def _param_array(v, prefix, layers):
    L = _L()
    return (L.BlockParams * layers)(*[_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, v, f"{prefix}{l}.") for l in range(layers)])


def block_case(lib, row):
    inp = block_inputs(row)
    desc = block_desc(row)
    p = C.byref(desc)
    bufs = _block_bufs(row, inp, 1, lib.egt_block_saved_bytes(p), lib.egt_block_workspace_bytes(p))

    def fwd(v):
        return lib.egt_block_fwd(p, _param_array(v, "p", 1), _ptr(v, "h"), _ptr(v, "e"), _ptr(v, "key_mask"), _ptr(v, "attn_mask"),
                                 _ptr(v, "rand_mask"), _ptr(v, "h_out"), _ptr(v, "e_out"), _ptr(v, "saved"), _ptr(v, "ws"), _stream())

    def bwd(v):
        return lib.egt_block_bwd(p, _param_array(v, "p", 1), _ptr(v, "h"), _ptr(v, "e"), _ptr(v, "key_mask"), _ptr(v, "attn_mask"),
                                 _ptr(v, "rand_mask"), _ptr(v, "saved"), _ptr(v, "d_h_out"), _ptr(v, "d_e_out"), _ptr(v, "d_h"),
                                 _ptr(v, "d_e"), _param_array(v, "g", 1), _ptr(v, "ws"), _stream())
    aliases = [] if "null_deo" in row[6] else [{"d_e": "d_e_out"}]          # "d_e may alias d_e_out"
    return Case(row[0], bufs, [fwd, bwd], aliases, row=row, inp=inp, desc=desc, layers=1, fwd_form=row[7], bwd_form=row[8])


def stack_case(lib, row, layers=STACK_LAYERS):
    inp = block_inputs(row, layers)
    desc = block_desc(row)
    p = C.byref(desc)
    bufs = _block_bufs(row, inp, layers, lib.egt_stack_saved_bytes(p, layers), lib.egt_stack_workspace_bytes(p, layers))

    def fwd(v):
        return lib.egt_stack_fwd(p, layers, _param_array(v, "p", layers), _ptr(v, "h"), _ptr(v, "e"), _ptr(v, "key_mask"),
                                 _ptr(v, "attn_mask"), _ptr(v, "h_out"), _ptr(v, "e_out"), _ptr(v, "saved"), _ptr(v, "ws"), _stream())

    def bwd(v):
        return lib.egt_stack_bwd(p, layers, _param_array(v, "p", layers), _ptr(v, "h"), _ptr(v, "e"), _ptr(v, "key_mask"),
                                 _ptr(v, "attn_mask"), _ptr(v, "saved"), _ptr(v, "d_h_out"), _ptr(v, "d_e_out"), _ptr(v, "d_h"),
                                 _ptr(v, "d_e"), _param_array(v, "g", layers), _ptr(v, "ws"), _stream())
    return Case(row[0], bufs, [fwd, bwd], [{"d_e": "d_e_out"}], row=row, inp=inp, desc=desc, layers=layers, fwd_form=row[7],
                bwd_form=row[8])


def layer_seed(seed, layer):
    return (seed ^ (0x9E3779B97F4A7C15 * (layer + 1))) & 0xFFFFFFFFFFFFFFFF


def block_oracle(case):
    """fp64 oracle of a block / stack case on the case's (storage-rounded) inputs: dict of outputs by buffer name"""
    from oracle import egt_oracle as O, rng_ref
    row, inp, layers = case.claims["row"], case.claims["inp"], case.claims["layers"]
    _, B, N, d, De, bf16, extras, _, _ = row
    static = "static" in extras
    if inp["rand_mask"] is not None:
        rms = [inp["rand_mask"].bool()]
    else:
        seeds = [SEED] if case.name in [r[0] for r in BLOCK_TABLE] else [layer_seed(SEED, l) for l in range(layers)]
        rms = [torch.from_numpy(rng_ref.random_mask(s, B, N, 8, RAND_P)) for s in seeds]
    h = inp["h"].double().requires_grad_()
    e = inp["e"].double().requires_grad_()
    ps = [{k: t.double().requires_grad_() for k, t in zip(BLOCK_ORACLE_NAMES, lp)} for lp in inp["params"]]
    kw = dict(num_heads=8, edge_channel_type="bias" if static else "residual",
              attn_mask=None if inp["attn_mask"] is None else inp["attn_mask"].double())
    h2, e2 = O.stack_forward(h, e, inp["key_mask"].bool(), ps, rand_masks=rms, **kw)
    loss = (h2 * inp["dh"].double()).sum()
    if "null_deo" not in extras:
        loss = loss + (e2 * inp["de"].double()).sum()
    flat = [t for lp in ps for t in lp.values()]
    gr = torch.autograd.grad(loss, [h, e] + flat, allow_unused=True)
    out = {"h_out": (h2.detach(), False), "d_h": (gr[0], True), "d_e": (gr[1], True)}
    if not static:
        out["e_out"] = (e2.detach(), False)
    gi = iter(gr[2:])
    for l in range(layers):
        for f in _L().BLOCK_PARAM_FIELDS:
            gval = next(gi)
            if gval is not None:
                out[f"g{l}.{f}"] = (gval, True)
    return out            # name -> (reference, is a gradient)


# ------------------------------------------------------------------------------------------------ inner op -----
ATTN_NAMES = ("gated_d6_n37", "randmask_dropout", "scale_log_vn2", "ungated_noedge", "gated_allmasked")
ROWSTATS_RESERVED = ("rowstats [B,N,H,4] fp32 (softmax max, softmax sum, gate degree, reserved)", lambda t: torch.arange(4, device=t.device) == 3)


def _u8(t):
    return None if t is None else t.to(torch.uint8)


def _attn_bufs(inp, B, N, H, d, a_tild):
    bufs = [Buf("qkv", IN, inp["QKV"], graphs=B), Buf("d_v_att", IN, inp["dV"], graphs=B), Buf("d_h_ext", IN, inp["dH"], graphs=B)]
    for k, src, grad in (("E", inp["E"], True), ("G", inp["G"], True), ("key_mask", _u8(inp["mask"]), False), ("attn_mask", inp["M"], False),
                         ("rand_mask", _u8(inp["rand_mask"]), False), ("drop_keep", _u8(inp.get("drop_keep")), False)):
        if src is not None:
            bufs.append(Buf(k, IN, src, graphs=B))
            if grad:
                bufs.append(Buf("d_" + k, OUT, dtype=torch.float32, shape=src.shape, graphs=B))
    bufs += [Buf("v_att", OUT, dtype=torch.float32, shape=(B, N, d * H), graphs=B),
             Buf("h_hat", OUT, dtype=torch.float32, shape=(B, N, N, H), graphs=B),
             Buf("d_qkv", OUT, dtype=torch.float32, shape=inp["QKV"].shape, graphs=B)]
    if a_tild:
        bufs.append(Buf("a_tild", OUT, dtype=torch.float32, shape=(B, N, N, H), graphs=B))
    return bufs


def _attn_oracle(inp, attrs):
    def f():
        import cases as CS
        ref = CS.attn_oracle(inp, attrs)
        out = {"v_att": (ref["V_att"], False), "h_hat": (ref["H_hat"], False), "a_tild": (ref["A_tild"], False), "d_qkv": (ref["dQKV"], True)}
        if ref["dE"] is not None:
            out["d_E"] = (ref["dE"], True)
        if ref["dG"] is not None:
            out["d_G"] = (ref["dG"], True)
        return out
    return f


def attn_case(lib, name, a_tild):
    import cases as CS
    from egt_amd.functional import AttnConfig, _attn_desc
    inp, attrs, c = CS.make_attn_case(name)
    B, N, H, d = c["B"], c["N"], c["H"], c["d"]
    stochastic = inp["rand_mask"] is not None or inp["drop_keep"] is not None
    cfg = AttnConfig(num_heads=H, clip_logits_value=attrs["clip_logits_value"], scale_degree=attrs["scale_degree"],
                     scaler_type=attrs["scaler_type"], num_virtual_nodes=attrs["num_virtual_nodes"],
                     random_mask_prob=0.5 if inp["rand_mask"] is not None else 0.0, attn_dropout=attrs["attn_dropout"],
                     training=stochastic, seed=7, need_a_tild=a_tild)
    desc = _attn_desc(cfg, B, N, d, inp["E"] is not None, inp["G"] is not None, inp["M"] is not None)
    p = C.byref(desc)
    bufs = _attn_bufs(inp, B, N, H, d, a_tild)
    bufs += [Buf("rowstats", CARRIED, dtype=torch.float32, shape=(B, N, H, 4), graphs=B, compare=True, const_after=0, exempt=ROWSTATS_RESERVED),
             Buf("ws", SCRATCH, nbytes=lib.egt_attn_bwd_workspace_bytes(p), graphs=B)]
    common = ("qkv", "E", "G", "key_mask", "attn_mask", "rand_mask", "drop_keep")

    def fwd(v):
        return lib.egt_attn_fwd(p, *[_ptr(v, k) for k in common], _ptr(v, "v_att"), _ptr(v, "h_hat"), _ptr(v, "a_tild"),
                                _ptr(v, "rowstats"), _stream())

    def bwd(v):
        return lib.egt_attn_bwd(p, *[_ptr(v, k) for k in common], _ptr(v, "v_att"), _ptr(v, "rowstats"), _ptr(v, "d_v_att"),
                                _ptr(v, "d_h_ext"), _ptr(v, "d_qkv"), _ptr(v, "d_E"), _ptr(v, "d_G"), _ptr(v, "ws"), _stream())
    return Case(f"attn_{name}{'_atild' if a_tild else ''}", bufs, [fwd, bwd], desc=desc, oracle=_attn_oracle(inp, attrs))


def mfma_case(lib, B, N, d, shared):
    L = _L()
    from egt_amd.functional import AttnConfig, _attn_desc
    H = 8
    g = _gen(f"mfma{B}.{N}.{d}")
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[B - 1, N - 8:] = False
    inp = dict(QKV=r(B, N, 3 * d * H) * 0.7, E=r(B, N, N, H), G=r(B, N, N, H), mask=mask, M=None, rand_mask=None, drop_keep=None,
               dV=r(B, N, d * H), dH=r(B, N, N, H))
    attrs = dict(num_heads=H, clip_logits_value=(-5.0, 5.0), scale_degree=False, scaler_type="log", num_virtual_nodes=0, attn_dropout=0.0)
    desc = _attn_desc(AttnConfig(), B, N, d, True, True, False)
    desc.reserved = L.ATTN_WS_SHARED if shared else 0
    p = C.byref(desc)
    bufs = _attn_bufs(inp, B, N, H, d, False)
    # an output of the pair (forward, backward), compared in full; the backward may change slot 3 and nothing else
    bufs.append(Buf("rowstats", CARRIED, dtype=torch.float32, shape=(B, N, H, 4), graphs=B, compare=True, const_after=0,
                    rmw={1: ("rowstats is read and its 4th slot written", ROWSTATS_RESERVED[1])}))
    if shared:
        bufs.append(Buf("ws", CARRIED, nbytes=lib.egt_attn_mfma_workspace_bytes(p), graphs=B))
    else:       # the forward-only size query for the forward alone
        bufs += [Buf("ws_fwd", SCRATCH, nbytes=lib.egt_attn_mfma_fwd_workspace_bytes(p), graphs=B),
                 Buf("ws", SCRATCH, nbytes=lib.egt_attn_mfma_workspace_bytes(p), graphs=B)]
    common = ("qkv", "E", "G", "key_mask", "attn_mask", "rand_mask")

    def fwd(v):
        return lib.egt_attn_mfma_fwd(p, *[_ptr(v, k) for k in common], _ptr(v, "v_att"), _ptr(v, "h_hat"), _ptr(v, "rowstats"),
                                     _ptr(v, "ws" if shared else "ws_fwd"), _stream())

    def bwd(v):
        return lib.egt_attn_mfma_bwd(p, *[_ptr(v, k) for k in common], _ptr(v, "v_att"), _ptr(v, "rowstats"), _ptr(v, "d_v_att"),
                                     _ptr(v, "d_h_ext"), _ptr(v, "d_qkv"), _ptr(v, "d_E"), _ptr(v, "d_G"), _ptr(v, "ws"), _stream())
    return Case(f"mfma_b{B}_n{N}_d{d}{'_shared' if shared else ''}", bufs, [fwd, bwd], desc=desc, oracle=_attn_oracle(inp, attrs),
                supported=lambda: lib.egt_attn_mfma_supported(p, 0))


# --------------------------------------------------------------------------------------------- pair operator -----
PAIR_SLOTS = (0, 1, 2, 3, 4, 5, 12, 13)


def pair_case(lib, B, N, real, shared):
    L = _L()
    from oracle import egt_oracle as O
    d, De, H = 64, 32, 8
    g = _gen(f"pair{B}.{N}")
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    km = torch.ones(B, N, dtype=torch.uint8)
    km[B - 1, real:] = 0
    inp = dict(qkv=r(B, N, 3 * d * H) * 0.7, e=r(B, N, N, De) * 1.3 + 0.2, key_mask=km, d_v_att=r(B, N, d * H), d_e_out=r(B, N, N, De))
    allp = O.init_block_params(d * H, De, H, dtype=torch.float32, generator=g, randomize_norm=True)
    params = {L.BLOCK_PARAM_FIELDS[i]: allp[BLOCK_ORACLE_NAMES[i]] for i in PAIR_SLOTS}
    desc = L.BlockDesc(B=B, N=N, H=H, d=d, De=De, dtype=L.EGT_F32, flags=L.BF_GATE | L.BF_CLIP | L.BF_TRAINING, clip_lo=-5.0, clip_hi=5.0,
                       random_mask_prob=RAND_P, ln_eps=1e-3, reserved=L.ATTN_WS_SHARED if shared else 0, seed=SEED, seed_device=None)
    p = C.byref(desc)
    bufs = [Buf(k, IN, t, graphs=B) for k, t in inp.items()]
    for f, t in params.items():
        bufs += [Buf("p." + f, IN, t, ptr=PARAM), Buf("g." + f, OUT, dtype=torch.float32, shape=t.shape, ptr=SINK)]
    bufs += [Buf("v_att", OUT, dtype=torch.float32, shape=(B, N, d * H), graphs=B),
             Buf("e_out", OUT, dtype=torch.float32, shape=inp["e"].shape, graphs=B),
             Buf("d_qkv", OUT, dtype=torch.float32, shape=inp["qkv"].shape, graphs=B),
             Buf("d_e", OUT, dtype=torch.float32, shape=inp["e"].shape, graphs=B),
             Buf("rowstats", CARRIED, dtype=torch.float32, shape=(B, N, H, 4), graphs=B, compare=True, const_after=0,
                 rmw={1: ("rowstats [B,N,H,4] is the forward's output (read; slot 3 written)", ROWSTATS_RESERVED[1])}),
             Buf("ws", CARRIED if shared else SCRATCH, nbytes=lib.egt_pair_workspace_bytes(p), graphs=B)]

    def fwd(v):
        return lib.egt_pair_fwd(p, C.byref(_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, v, "p.")), _ptr(v, "qkv"), _ptr(v, "e"),
                                _ptr(v, "key_mask"), _ptr(v, "v_att"), _ptr(v, "e_out"), _ptr(v, "rowstats"), _ptr(v, "ws"), _stream())

    def bwd(v):
        return lib.egt_pair_bwd(p, C.byref(_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, v, "p.")), _ptr(v, "qkv"), _ptr(v, "e"),
                                _ptr(v, "key_mask"), _ptr(v, "v_att"), _ptr(v, "rowstats"), _ptr(v, "d_v_att"), _ptr(v, "d_e_out"),
                                _ptr(v, "d_qkv"), _ptr(v, "d_e"), C.byref(_struct(L.BlockParams, L.BLOCK_PARAM_FIELDS, v, "g.")),
                                _ptr(v, "ws"), _stream())

    def wrapper(dev):
        from egt_amd.pair import _PairOp
        wd = L.BlockDesc.from_buffer_copy(desc)
        qkv, e = inp["qkv"].to(dev).requires_grad_(), inp["e"].to(dev).requires_grad_()
        ps = [t.to(dev).requires_grad_() for t in params.values()]
        v_att, e_out = _PairOp.apply(qkv, e, km.to(dev), wd, *ps)
        torch.autograd.backward([v_att, e_out], [inp["d_v_att"].to(dev), inp["d_e_out"].to(dev)])
        out = {"v_att": v_att.detach(), "e_out": e_out.detach(), "d_qkv": qkv.grad, "d_e": e.grad}
        out.update({"g." + f: t.grad for f, t in zip(params, ps)})
        return out
    return Case(f"pair_b{B}_n{N}{'_shared' if shared else ''}", bufs, [fwd, bwd], [{"d_e": "d_e_out"}], desc=desc, wrapper=wrapper,
                supported=lambda: lib.egt_pair_supported(p))


# -------------------------------------------------------------------------------------------------- edge ops -----
EDGE_PARAMS = ("gamma", "beta", "Wg", "bg", "We", "be", "Wr", "br")


def _edge_inputs(De, name):
    g = _gen(name)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    shape = (2, 13, 13)
    return g, r, shape


def edge_proj_case(lib, De, ln, gates, acc):
    L = _L()
    g, r, shape = _edge_inputs(De, f"proj{De}")
    act = None if ln else "elu"
    inp = dict(e=r(*shape, De) * 1.3 + 0.2, We=r(De, 8) * 0.3, be=r(8) * 0.2, d_E=r(*shape, 8))
    if ln:
        inp.update(gamma=1.0 + 0.2 * r(De), beta=0.2 * r(De))
    if gates:
        inp.update(Wg=r(De, 8) * 0.3, bg=r(8) * 0.2, d_G=r(*shape, 8))
    if acc:
        inp["d_e_base"] = r(*shape, De)
    rows = shape[0] * shape[1] * shape[2]
    desc = L.EdgeDesc(rows=rows, De=De, H=8, dtype=L.EGT_F32, flags=(L.EP_LAYERNORM if ln else 0) | (L.EP_GATES if gates else 0),
                      act=L.ACT_ELU if act else L.ACT_NONE, act_alpha=0.0, ln_eps=1e-3, reserved=0)
    p = C.byref(desc)
    bufs = [Buf(k, IN, t, graphs=shape[0], ptr=PARAM if k in EDGE_PARAMS else None) for k, t in inp.items()]
    bufs += [Buf("E_out", OUT, dtype=torch.float32, shape=(*shape, 8), graphs=2), Buf("d_e", OUT, dtype=torch.float32, shape=(*shape, De), graphs=2),
             Buf("d_We", OUT, dtype=torch.float32, shape=(De, 8), ptr=SINK), Buf("d_be", OUT, dtype=torch.float32, shape=(8,), ptr=SINK),
             Buf("ws", SCRATCH, nbytes=lib.egt_edge_proj_bwd_workspace_bytes(p), graphs=2)]
    if ln:
        bufs += [Buf("d_gamma", OUT, dtype=torch.float32, shape=(De,), ptr=SINK), Buf("d_beta", OUT, dtype=torch.float32, shape=(De,), ptr=SINK)]
    if gates:
        bufs += [Buf("G_out", OUT, dtype=torch.float32, shape=(*shape, 8), graphs=2), Buf("d_Wg", OUT, dtype=torch.float32, shape=(De, 8), ptr=SINK),
                 Buf("d_bg", OUT, dtype=torch.float32, shape=(8,), ptr=SINK)]

    def fwd(v):
        return lib.egt_edge_proj_fwd(p, *[_ptr(v, k) for k in ("e", "gamma", "beta", "Wg", "bg", "We", "be", "G_out", "E_out")], _stream())

    def bwd(v):
        head = [_ptr(v, k) for k in ("e", "gamma", "beta", "Wg", "We", "E_out", "d_G", "d_E")]
        tail = [_ptr(v, k) for k in ("d_e", "d_gamma", "d_beta", "d_Wg", "d_bg", "d_We", "d_be", "ws")]
        if acc:
            return lib.egt_edge_proj_bwd_acc(p, *head, _ptr(v, "d_e_base"), *tail, _stream())
        return lib.egt_edge_proj_bwd(p, *head, *tail, _stream())

    def wrapper(dev):
        from egt_amd.functional import edge_proj
        t = {k: x.to(dev).requires_grad_() for k, x in inp.items() if not k.startswith("d_")}
        res = edge_proj(t["e"], t.get("gamma"), t.get("beta"), t.get("Wg"), t.get("bg"), t["We"], t["be"], use_ln=ln, edge_activation=act,
                        passthrough=acc)
        outs, ups = [res[1]], [inp["d_E"].to(dev)]
        if gates:
            outs.append(res[0]); ups.append(inp["d_G"].to(dev))
        if acc:
            outs.append(res[2]); ups.append(inp["d_e_base"].to(dev))
        torch.autograd.backward(outs, ups)
        out = {"E_out": res[1].detach(), "d_e": t["e"].grad, "d_We": t["We"].grad, "d_be": t["be"].grad}
        if ln:
            out.update(d_gamma=t["gamma"].grad, d_beta=t["beta"].grad)
        if gates:
            out.update(G_out=res[0].detach(), d_Wg=t["Wg"].grad, d_bg=t["bg"].grad)
        return out
    return Case(f"edge_proj{'_acc' if acc else ''}_de{De}{'_ln' if ln else ''}{'_gates' if gates else ''}", bufs, [fwd, bwd],
                [{"d_e": "d_e_base"}] if acc else [], desc=desc, wrapper=wrapper)          # "d_e_base ... may alias d_e"


def edge_update_case(lib, De):
    L = _L()
    g, r, shape = _edge_inputs(De, f"upd{De}")
    inp = dict(e=r(*shape, De), h_hat=r(*shape, 8), Wr=r(8, De) * 0.3, br=r(De) * 0.2, d_e_out=r(*shape, De))
    desc = L.EdgeDesc(rows=shape[0] * shape[1] * shape[2], De=De, H=8, dtype=L.EGT_F32, flags=0, act=L.ACT_NONE, act_alpha=0.0, ln_eps=1e-3,
                      reserved=0)
    p = C.byref(desc)
    bufs = [Buf(k, IN, t, graphs=2, ptr=PARAM if k in EDGE_PARAMS else None) for k, t in inp.items()]
    bufs += [Buf("e_out", OUT, dtype=torch.float32, shape=(*shape, De), graphs=2), Buf("d_h_hat", OUT, dtype=torch.float32, shape=(*shape, 8), graphs=2),
             Buf("d_Wr", OUT, dtype=torch.float32, shape=(8, De), ptr=SINK), Buf("d_br", OUT, dtype=torch.float32, shape=(De,), ptr=SINK),
             Buf("ws", SCRATCH, nbytes=lib.egt_edge_update_bwd_workspace_bytes(p), graphs=2)]

    def fwd(v):
        return lib.egt_edge_update_fwd(p, *[_ptr(v, k) for k in ("e", "h_hat", "Wr", "br", "e_out")], _stream())

    def bwd(v):
        return lib.egt_edge_update_bwd(p, *[_ptr(v, k) for k in ("d_e_out", "h_hat", "Wr", "d_h_hat", "d_Wr", "d_br", "ws")], _stream())

    def wrapper(dev):
        from egt_amd.functional import edge_update
        t = {k: x.to(dev).requires_grad_() for k, x in inp.items() if k != "d_e_out"}
        out = edge_update(t["e"], t["h_hat"], t["Wr"], t["br"])
        out.backward(inp["d_e_out"].to(dev))
        return {"e_out": out.detach(), "d_h_hat": t["h_hat"].grad, "d_Wr": t["Wr"].grad, "d_br": t["br"].grad}
    return Case(f"edge_update_de{De}", bufs, [fwd, bwd], desc=desc, wrapper=wrapper)


# ------------------------------------------------------------------------------------------------ channel FFN -----
def ffn_case(lib, W, rows, bf16, matmul, prepared):
    L = _L()
    import cases as CS
    g = _gen(f"ffn{W}")
    H2 = 2 * W
    lim = (6.0 / (W + H2)) ** 0.5
    rn = lambda *s: torch.randn(*s, generator=g)
    params = {"norm_gamma": 1.0 + 0.3 * rn(W), "norm_beta": 0.3 * rn(W), "lr1_kernel": (torch.rand(W, H2, generator=g) * 2 - 1) * lim,
              "lr1_bias": 0.2 * rn(H2), "lr2_kernel": (torch.rand(H2, W, generator=g) * 2 - 1) * lim, "lr2_bias": 0.2 * rn(W)}
    sdt = torch.bfloat16 if bf16 else torch.float32
    inp = {"x": (rn(rows, W) * 1.5 + 0.2).to(sdt), "dy": rn(rows, W).to(sdt)}
    mk = lambda flags: L.FfnDesc(rows=rows, width=W, dtype=L.EGT_BF16 if bf16 else L.EGT_F32, activation=L.ACT_ELU, ln_eps=1e-3,
                                 matmul={"f32": L.MM_F32, "bf16x3": L.MM_BF16X3}[matmul], flags=flags)
    desc, bdesc = mk(0), mk(L.FFN_WS_PREPARED if prepared else 0)
    p, bp = C.byref(desc), C.byref(bdesc)
    bufs = [Buf("x", IN, inp["x"]), Buf("dy", IN, inp["dy"]), Buf("y", OUT, dtype=sdt, shape=(rows, W)), Buf("dx", OUT, dtype=sdt, shape=(rows, W)),
            Buf("ws", CARRIED if prepared else SCRATCH, nbytes=lib.egt_ffn_workspace_bytes(p))]
    for f, t in params.items():
        bufs += [Buf("p." + f, IN, t, ptr=PARAM), Buf("g." + f, OUT, dtype=torch.float32, shape=t.shape, ptr=SINK)]

    def fwd(v):
        return lib.egt_ffn_fwd(p, C.byref(_struct(L.FfnParams, L.FFN_PARAM_FIELDS, v, "p.")), _ptr(v, "x"), _ptr(v, "y"), _ptr(v, "ws"), _stream())

    def bwd(v):
        return lib.egt_ffn_bwd(bp, C.byref(_struct(L.FfnParams, L.FFN_PARAM_FIELDS, v, "p.")), _ptr(v, "x"), _ptr(v, "dy"), _ptr(v, "dx"),
                               C.byref(_struct(L.FfnParams, L.FFN_PARAM_FIELDS, v, "g.")), _ptr(v, "ws"), _stream())

    def oracle():
        ref = CS.ffn_oracle({"x": inp["x"].float(), "dy": inp["dy"].float()}, params, {"act": "elu"})
        out = {"y": (ref["y"], False), "dx": (ref["dx"], True)}
        out.update({"g." + f: (t, True) for f, t in ref["dparams"].items()})
        return out
    return Case(f"ffn_w{W}_{'bf16' if bf16 else 'fp32'}_{matmul}{'_prepared' if prepared else ''}", bufs, [fwd, bwd], [{"dx": "dy"}],
                desc=desc, oracle=oracle, bf16=bf16, supported=lambda: lib.egt_ffn_supported(p))       # "dx may alias dy"


# --------------------------------------------------------------------------------------------- edge embedding -----
# (B, N, De, K, V, F): V rows of fm_table, F real-valued features
EMBED_TABLE = [(2, 19, 8, 4, 4, 0), (3, 37, 64, 16, 5, 0), (1, 21, 48, 1, 4, 0),
               (2, 33, 12, 3, 4, 2),          # De / 4 = 3 is no power of two: idle channel lanes in the backward
               (176, 37, 8, 3, 4, 0),         # two column tiles per k_hop_chain workgroup
               (1, 200, 8, 3, 4, 0)]          # k_hop_first / k_hop_step
VN_TABLE = [(nv, De) for nv in (1, 3, 16) for De in (8, 64)]
EMBED_PARAMS = ("fm_table", "adj_kernel", "adj_bias", "vn_table")


def embed_case(lib, B, N, De, K, V, F, bf16, nv=0):
    L = _L()
    g = _gen(f"embed{B}.{N}.{De}.{nv}")
    rn = lambda *s: torch.randn(*s, generator=g)
    sizes = torch.randint(max(1, N // 2), N + 1, (B,), generator=g)
    sizes[0] = N
    real = torch.arange(N)[None, :] < sizes[:, None]
    pair = (real[:, :, None] & real[:, None, :])
    adj = (torch.rand(B, N, N, generator=g) > 0.8).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float() * pair.float()
    fm = torch.where(adj > 0, torch.randint(0, V - 1, (B, N, N), generator=g), torch.tensor(-1)).to(torch.int32)
    sdt = torch.bfloat16 if bf16 else torch.float32
    NO = N + nv
    inp = dict(feature_matrix=fm, graph_matrix=adj, fm_table=rn(V, De) * 0.5, adj_kernel=rn(K + F, De) * 0.3, adj_bias=rn(De) * 0.2,
               d_e=rn(B, NO, NO, De).to(sdt))
    if F:
        ff = rn(B, N, N, F)
        ff[~pair] = -1.0                           # Masking(mask_value): a pair whose features all equal it contributes 0
        inp["float_features"] = ff
    if nv:
        inp["vn_table"] = rn(nv, De) * 0.5
    desc = L.EmbedDesc(B=B, N=N, De=De, upto_hop=K, clip_hops=1, num_edge_features=V - 1, dtype=L.EGT_BF16 if bf16 else L.EGT_F32,
                       num_float_features=F, mask_value=-1.0, reserved=0)
    p = C.byref(desc)
    ws = lib.egt_edge_embed_vn_workspace_bytes(p, nv) if nv else lib.egt_edge_embed_workspace_bytes(p)
    bufs = [Buf(k, IN, t, graphs=B if t.shape[0] == B and t.dim() > 2 else 1, ptr=PARAM if k in EMBED_PARAMS else None)
            for k, t in inp.items()]
    bufs += [Buf("hops", CARRIED, dtype=torch.float32, shape=(K + F, B, N, N), graphs=K + F, const_after=0),
             Buf("e_out", OUT, dtype=sdt, shape=(B, NO, NO, De), graphs=B), Buf("ws", SCRATCH, nbytes=ws, graphs=B)]
    assert bufs[-3].nbytes == lib.egt_edge_embed_hops_bytes(p)
    for k in EMBED_PARAMS[:4 if nv else 3]:
        bufs.append(Buf("d_" + k, OUT, dtype=torch.float32, shape=inp[k].shape, ptr=SINK))
    fin = ("feature_matrix", "graph_matrix", "float_features", "fm_table", "adj_kernel", "adj_bias")

    def fwd(v):
        if nv:
            return lib.egt_edge_embed_vn_fwd(p, nv, *[_ptr(v, k) for k in fin + ("vn_table", "hops", "e_out")], _stream())
        return lib.egt_edge_embed_fwd(p, *[_ptr(v, k) for k in fin + ("hops", "e_out")], _stream())

    def bwd(v):
        head = [_ptr(v, k) for k in ("feature_matrix", "hops", "d_e", "d_fm_table", "d_adj_kernel", "d_adj_bias")]
        if nv:
            return lib.egt_edge_embed_vn_bwd(p, nv, *head, _ptr(v, "d_vn_table"), _ptr(v, "ws"), _stream())
        return lib.egt_edge_embed_bwd(p, *head, _ptr(v, "ws"), _stream())

    def wrapper(dev):
        from egt_amd.model import edge_embed
        t = {k: inp[k].to(dev).requires_grad_() for k in ("fm_table", "adj_kernel", "adj_bias") + (("vn_table",) if nv else ())}
        kw = {}
        kernel = t["adj_kernel"]
        if F:       # the wrapper takes the two Dense layers apart: same rows, same sum
            kw = dict(float_features=inp["float_features"].to(dev), float_kernel=kernel[K:], float_bias=torch.zeros(De, device=dev))
            kernel = kernel[:K]
        e, hops = edge_embed(fm.to(dev), adj.to(dev), t["fm_table"], kernel, t["adj_bias"], clip_hops=True, return_hops=True,
                             edge_dtype="bf16" if bf16 else "f32", virtual_edge_table=t.get("vn_table"), **kw)
        e.backward(inp["d_e"].to(dev))
        out = {"e_out": e.detach(), "hops": hops}
        out.update({"d_" + k: x.grad for k, x in t.items()})
        return out
    bufs[[b.name for b in bufs].index("hops")].compare = True
    tag = f"embed{'_vn%d' % nv if nv else ''}_b{B}_n{N}_de{De}_k{K}{'_f%d' % F if F else ''}_{'bf16' if bf16 else 'fp32'}"
    return Case(tag, bufs, [fwd, bwd], desc=desc, wrapper=wrapper,
                supported=lambda: (lib.egt_edge_embed_vn_supported(p, nv) if nv else lib.egt_edge_embed_supported(p)))


# ---------------------------------------------------------------------------------------------------- heads -----
def edge_head_case(lib, De, M0, M1, bf16):
    L = _L()
    B, N, Cc = 2, 19, 5
    g = _gen(f"ehead{De}.{M0}")
    rn = lambda *s: torch.randn(*s, generator=g)
    sdt = torch.bfloat16 if bf16 else torch.float32
    params = dict(zip(L.HEAD_PARAM_FIELDS, (1.0 + 0.2 * rn(De), 0.2 * rn(De), rn(De, M0) * 0.3, rn(M0) * 0.2, rn(M0, M1) * 0.3, rn(M1) * 0.2,
                                             rn(M1, Cc) * 0.3, rn(Cc) * 0.2)))
    inp = dict(e=(rn(B, N, N, De) * 1.3).to(sdt), target=torch.randint(0, Cc, (B, N, N), generator=g).to(torch.uint8), d_per_graph=rn(B))
    desc = L.HeadDesc(B=B, N=N, De=De, M0=M0, M1=M1, C=Cc, dtype=L.EGT_BF16 if bf16 else L.EGT_F32, activation=L.ACT_ELU, flags=L.EH_LAYERNORM,
                      ln_eps=1e-3, reserved=0)
    p = C.byref(desc)
    bufs = [Buf(k, IN, t, graphs=B) for k, t in inp.items()]
    for f, t in params.items():
        bufs += [Buf("p." + f, IN, t, ptr=PARAM), Buf("g." + f, OUT, dtype=torch.float32, shape=t.shape, ptr=SINK)]
    bufs += [Buf("per_graph_loss", OUT, dtype=torch.float32, shape=(B,)), Buf("d_e", OUT, dtype=sdt, shape=(B, N, N, De), graphs=B),
             Buf("ws", SCRATCH, nbytes=lib.egt_edge_head_workspace_bytes(p), graphs=B)]

    def fwd(v):
        return lib.egt_edge_head_fwd(p, C.byref(_struct(L.HeadParams, L.HEAD_PARAM_FIELDS, v, "p.")), _ptr(v, "e"), _ptr(v, "target"),
                                     _ptr(v, "per_graph_loss"), _ptr(v, "ws"), _stream())

    def bwd(v):
        return lib.egt_edge_head_bwd(p, C.byref(_struct(L.HeadParams, L.HEAD_PARAM_FIELDS, v, "p.")), _ptr(v, "e"), _ptr(v, "target"),
                                     _ptr(v, "d_per_graph"), _ptr(v, "d_e"), C.byref(_struct(L.HeadParams, L.HEAD_PARAM_FIELDS, v, "g.")),
                                     _ptr(v, "ws"), _stream())

    def wrapper(dev):
        from egt_amd.head import distance_head
        e = inp["e"].to(dev).requires_grad_()
        ps = [t.to(dev).requires_grad_() for t in params.values()]
        out = distance_head(e, inp["target"].to(dev), ps)
        out.backward(inp["d_per_graph"].to(dev))
        res = {"per_graph_loss": out.detach(), "d_e": e.grad}
        res.update({"g." + f: t.grad for f, t in zip(params, ps)})
        return res
    return Case(f"edge_head_de{De}_m{M0}_{'bf16' if bf16 else 'fp32'}", bufs, [fwd, bwd], desc=desc, wrapper=wrapper,
                supported=lambda: lib.egt_edge_head_supported(p))


def node_head_case(lib, W, Cc):
    L = _L()
    B, N = 2, 37
    M0, M1 = (24, 12) if W == 16 else (32, 16)
    g = _gen(f"nhead{W}.{Cc}")
    rn = lambda *s: torch.randn(*s, generator=g)
    params = dict(zip(L.NODE_HEAD_PARAM_FIELDS, (1.0 + 0.2 * rn(W), 0.2 * rn(W), rn(W, M0) * 0.3, rn(M0) * 0.2, rn(M0, M1) * 0.3, rn(M1) * 0.2,
                                                  rn(M1, Cc) * 0.3, rn(Cc) * 0.2)))
    mask = torch.ones(B, N, dtype=torch.uint8)
    mask[0, 30:] = 0
    mask[1, 5] = 0
    target = torch.randint(0, Cc, (B, N), generator=g).to(torch.int32)
    target[mask == 0] = -1
    inp = dict(h=rn(B, N, W), target=target, mask=mask, class_weights=torch.rand(Cc, generator=g) + 0.5, d_loss=torch.tensor([0.7]))
    desc = L.NodeHeadDesc(B=B, N=N, W=W, M0=M0, M1=M1, C=Cc, activation=L.ACT_ELU, flags=L.NH_LAYERNORM, ln_eps=1e-3, reserved=0)
    p = C.byref(desc)
    bufs = [Buf(k, IN, t) for k, t in inp.items()]
    for f, t in params.items():
        bufs += [Buf("p." + f, IN, t, ptr=PARAM), Buf("g." + f, OUT, dtype=torch.float32, shape=t.shape, ptr=SINK)]
    bufs += [Buf("stats", OUT, dtype=torch.float32, shape=(3,)), Buf("d_h", OUT, dtype=torch.float32, shape=(B, N, W), graphs=B),
             Buf("ws", SCRATCH, nbytes=lib.egt_node_head_workspace_bytes(p), graphs=B)]
    args = ("h", "target", "mask", "class_weights")

    def fwd(v):
        return lib.egt_node_head_fwd(p, C.byref(_struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, v, "p.")), *[_ptr(v, k) for k in args],
                                     _ptr(v, "stats"), _ptr(v, "ws"), _stream())

    def bwd(v):
        return lib.egt_node_head_bwd(p, C.byref(_struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, v, "p.")), *[_ptr(v, k) for k in args],
                                     _ptr(v, "d_loss"), _ptr(v, "d_h"), C.byref(_struct(L.NodeHeadParams, L.NODE_HEAD_PARAM_FIELDS, v, "g.")),
                                     _ptr(v, "ws"), _stream())

    def wrapper(dev):
        from egt_amd.node_head import node_head_loss
        h = inp["h"].to(dev).requires_grad_()
        ps = [t.to(dev).requires_grad_() for t in params.values()]
        stats = node_head_loss(h, target.to(dev), mask.to(dev), inp["class_weights"].to(dev), ps)
        stats.backward(torch.tensor([0.7, 0.0, 0.0], device=dev))
        res = {"stats": stats.detach(), "d_h": h.grad}
        res.update({"g." + f: t.grad for f, t in zip(params, ps)})
        return res
    return Case(f"node_head_w{W}_c{Cc}", bufs, [fwd, bwd], desc=desc, wrapper=wrapper, mask=mask,
                supported=lambda: lib.egt_node_head_supported(p))


def distance_target_case(lib, N):
    B, T = 2, 4
    g = _gen(f"dt{N}")
    adj = (torch.rand(B, N, N, generator=g) > 0.85).float()
    adj = ((adj + adj.transpose(1, 2)) > 0).float()
    bufs = [Buf("adj", IN, adj, graphs=B), Buf("target", OUT, dtype=torch.uint8, shape=(B, N, N), graphs=B)]

    def step(v):
        return lib.egt_distance_target(_ptr(v, "adj"), B, N, T, _ptr(v, "target"), _stream())

    def wrapper(dev):       # integer work: the host path of distance_target (fp64 sums of 0/1 products) is the reference, bit for bit
        from egt_amd.head import distance_target
        return {"target": distance_target(adj, T).to(dev)}
    return Case(f"distance_target_n{N}", bufs, [step], wrapper=wrapper)


# ------------------------------------------------------------------------------------------- mask producers -----
MASK_SHAPES = [(1, 1, 0), (3, 37, 0), (2, 9, 1)]          # (B, N, nv): tests/test_masks.py


def mask_cases(lib):
    out = []
    for B, N, nv in MASK_SHAPES:
        tag = f"b{B}_n{N}_nv{nv}"
        g = _gen("masks" + tag)
        feats = torch.randint(-1, 5, (B, N), generator=g).to(torch.int32)
        ffeat = torch.where(torch.rand(B, N, 1, generator=g) > 0.3, torch.randn(B, N, 3, generator=g), torch.tensor(-1.0)).contiguous()
        adj = (torch.rand(B, N, N, generator=g) > 0.5).float()
        NO = N + nv

        def f_int(v, B=B, N=N, nv=nv):
            return lib.egt_node_mask_from_features(_ptr(v, "features"), B, N, nv, _ptr(v, "mask"), _stream())

        def f_float(v, B=B, N=N, nv=nv):
            return lib.egt_node_mask_from_float_features(_ptr(v, "features"), B, N, 3, C.c_float(-1.0), nv, _ptr(v, "mask"), _stream())

        def f_edge(v, B=B, N=N, nv=nv):
            return lib.egt_constrained_edge_mask(_ptr(v, "adj"), B, N, 8, nv, _ptr(v, "M"), _stream())

        def f_sample(v, B=B, NO=NO, which=0):
            return lib.egt_mask_sample(which, C.c_uint64(SEED), C.c_float(0.3), B, NO, 8, _ptr(v, "out"), _stream())

        def f_keep(v, B=B, NO=NO):
            return f_sample(v, B, NO, 1)
        out += [Case("node_mask_" + tag, [Buf("features", IN, feats), Buf("mask", OUT, dtype=torch.uint8, shape=(B, NO))], [f_int]),
                Case("node_mask_float_" + tag, [Buf("features", IN, ffeat), Buf("mask", OUT, dtype=torch.uint8, shape=(B, NO))], [f_float]),
                Case("constrained_edge_mask_" + tag, [Buf("adj", IN, adj, graphs=B), Buf("M", OUT, dtype=torch.float32, shape=(B, NO, NO, 8), graphs=B)],
                     [f_edge]),
                Case("mask_sample_" + tag, [Buf("out", OUT, dtype=torch.uint8, shape=(B, NO, NO, 8), graphs=B)], [f_sample]),
                Case("dropout_keep_" + tag, [Buf("out", OUT, dtype=torch.uint8, shape=(B, NO, NO, 8), graphs=B)], [f_keep])]
    for count in (1, 37):
        words = torch.arange(count, dtype=torch.int64) * 0x0123456789ABCDE + 5

        def f_seed(v, count=count):
            return lib.egt_seed_advance(_ptr(v, "words"), count, C.c_uint64(0xD1B54A32D192ED03), _stream())
        out.append(Case(f"seed_advance_{count}", [Buf("words", INOUT, words)], [f_seed], words=words))
    return out


# ------------------------------------------------------------------------------------------------ all of them -----
def block_cases(lib, static=True):
    return [block_case(lib, r) for r in BLOCK_TABLE if static or "static" not in r[6]]


def stack_cases(lib):
    return [stack_case(lib, r) for r in STACK_TABLE]


def attn_cases(lib):
    return [attn_case(lib, n, a) for n in ATTN_NAMES for a in (False, True)]


def mfma_cases(lib):
    return [mfma_case(lib, B, N, d, s) for B, N, d in ((1, 37, 16), (2, 48, 64)) for s in (False, True)]


def pair_cases(lib):
    return [pair_case(lib, B, N, real, s) for B, N, real in ((1, 37, 29), (2, 48, 40)) for s in (False, True)]


def edge_cases(lib):
    out = [edge_proj_case(lib, De, ln, gt, acc) for De in (8, 48, 64) for ln in (False, True) for gt in (False, True) for acc in (False, True)]
    return out + [edge_update_case(lib, De) for De in (8, 48, 64)]


def ffn_cases(lib):
    out = []
    for W, rows in ((8, 1001), (16, 333), (48, 333), (64, 333)):
        for bf16 in (False, True):
            for mm in (("f32",) if W == 8 else ("f32", "bf16x3")):          # width 8: exact fp32 products only
                for prepared in (False, True):
                    out.append(ffn_case(lib, W, rows, bf16, mm, prepared))
    return out


def embed_cases(lib):
    out = [embed_case(lib, *r, bf16) for r in EMBED_TABLE for bf16 in (False, True)]
    return out + [embed_case(lib, 2, 19, De, 4, 4, 0, bf16, nv) for nv, De in VN_TABLE for bf16 in (False, True)]


def head_cases(lib):
    out = [edge_head_case(lib, De, M0, M1, bf16) for De in (8, 64) for M0, M1 in ((24, 12), (32, 16)) for bf16 in (False, True)]
    out += [node_head_case(lib, W, Cc) for W in (16, 64) for Cc in (2, 6)]
    return out + [distance_target_case(lib, N) for N in (1, 37, 192)]


FAMILIES = {"block": block_cases, "stack": stack_cases, "attn": attn_cases, "mfma": mfma_cases, "pair": pair_cases, "edge": edge_cases,
            "ffn": ffn_cases, "embed": embed_cases, "head": head_cases, "mask": mask_cases}


def all_cases(lib):
    for fam in FAMILIES.values():
        yield from fam(lib)
