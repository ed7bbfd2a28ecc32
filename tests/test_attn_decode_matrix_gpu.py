"""Every decode-attention instantiation against the fp64 reference.

Each case calls ops.attn_decode once and checks (1) attn_error_ok against
attn_reference's fp64 reference, (2) the appended K/V row, (3) that nothing
else in the pools (and scale tables) changed, (4) that `out` is written at
exactly n_batch * n_head * hs elements.  The reference must first satisfy
the probe precondition (every planted key carries weight in [0.02, 0.5]);
tests/test_attn_reference_cpu.py shows without a GPU that the metric then
catches a dropped key, a wrong rope, a stale V row, a wrong stride or a
mis-weighted chunk.

Case -> instantiation map.  Every family below is parametrised over
path in {block, split} x kv in {bf16, fp8}, i.e. over

    attn_decode_block_kernel<QPK, HS, BATCH, KV8>   (path=block)
    attn_decode_kernel<QPK, HS, BATCH, KV8> + attn_combine_kernel
                                                    (path=split, force_split=1)

  family      BATCH  (QPK, HS)                       what it is for
  geom        0      all 15 of {1,2,4,8,16} x        per-geometry PV maps (ODIM =
                     {64,128,256}; + rope_ne 0/16    QPK*HS/64 from 1 to 64), partial
                     on three, n_kv=8, scale=0.3     rotary, no rope, grid size, scale
  s_edge      0      (4,128), block only             empty waves, partial last tile,
                                                     the V row clamp, the last pool row
  chunk_edge  0      (4,128), split only             kpc steps, n_act 1/65/193/256,
                                                     pos on a chunk's first key
  mode        0      (4,128)                         online-softmax rescale (alpha)
  batched     1      (4,128), n_batch 3 and 1        per-sample pos/slot, batch strides
  implicit    0      (4,128), max_seq=8192, split    dispatch by max_seq alone
  guard       -      -                               n_chunks in {6, 260} is refused
"""

from dataclasses import dataclass, field

import pytest
import torch

from attn_reference import (attn_error_ok, attn_error_ratio,
                            bf16_ulp_distance, fp8_decode, keys_per_chunk,
                            make_case, pick_probes)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64  # bf16 elements after `out` that must stay untouched


@dataclass
class Spec:
    name: str
    family: str
    kw: dict                 # make_case arguments (without kv8)
    n_chunks: int = 8
    paths: tuple = ("block", "split")
    force_split: bool = True  # for path == "split"
    extra: dict = field(default_factory=dict)


def _single(name, family, qpk, n_kv, hs, S, max_seq, cand, n_chunks=8,
            paths=("block", "split"), seed=0, force_split=True, **kw):
    pos = S - 1
    probes = pick_probes(S, [pos + c if c < 0 else c for c in cand] + [pos])
    return Spec(name, family,
                dict(qpk=qpk, n_kv=n_kv, hs=hs, pos=pos, max_seq=max_seq,
                     probes=probes, seed=seed, **kw),
                n_chunks, paths, force_split)


def _specs():
    out = []
    # ---- geometry sweep: S=83, max_seq=128, n_chunks=8 -------------------
    cand = [0, 15, 16, 64, -1]
    seed = 100
    for qpk in (1, 2, 4, 8, 16):
        for hs in (64, 128, 256):
            seed += 1
            out.append(_single(f"geom-q{qpk}-h{hs}", "geom", qpk, 2, hs, 83,
                               128, cand, seed=seed))
    for qpk, hs in ((1, 64), (4, 128), (16, 256)):
        for ne in (0, 16):
            seed += 1
            out.append(_single(f"geom-q{qpk}-h{hs}-rope{ne}", "geom", qpk,
                               2, hs, 83, 128, cand, seed=seed, rope_ne=ne))
    out.append(_single("geom-q4-h128-nkv8", "geom", 4, 8, 128, 83, 128, cand,
                       seed=130))
    out.append(_single("geom-q4-h128-scale0.3", "geom", 4, 2, 128, 83, 128,
                       cand, seed=131, scale=0.3))
    # ---- block-local S edges ----------------------------------------------
    cand = [0, 15, 16, 63, 64, -1]
    for i, S in enumerate((1, 2, 16, 17, 63, 64, 65, 127, 128)):
        out.append(_single(f"s_edge-S{S}", "s_edge", 4, 2, 128, S, 128, cand,
                           paths=("block",), seed=200 + i))
    out.append(_single("s_edge-S4096", "s_edge", 4, 2, 128, 4096, 4096, cand,
                       paths=("block",), seed=210))
    # ---- split-S chunk edges ----------------------------------------------
    i = 0
    for n_chunks, Ss, max_seq in ((4, (1, 17, 64, 65), 128),
                                  (16, (16, 256, 257, 300), 512),
                                  (128, (1024, 1025, 1040), 2048),
                                  (256, (3073, 4096), 4096)):
        for S in Ss:
            kpc = keys_per_chunk(S, n_chunks)
            own = ((S - 1) // kpc) * kpc
            out.append(_single(f"chunk_edge-c{n_chunks}-S{S}", "chunk_edge",
                               4, 2, 128, S, max_seq,
                               [0, kpc - 1, kpc, own, -1], n_chunks,
                               paths=("split",), seed=300 + i))
            i += 1
    # pos is exactly a chunk's first key: S=33, 4 chunks -> kpc=16, pos=32
    # opens chunk 2, whose only key is the current one and which owns the
    # append
    assert keys_per_chunk(33, 4) == 16
    out.append(_single("chunk_edge-c4-S33-pos-first", "chunk_edge", 4, 2,
                       128, 33, 128, [0, 15, 16, 31], 4, paths=("split",),
                       seed=320))
    # ---- softmax modes ------------------------------------------------------
    for i, mode in enumerate(("ascending", "descending", "outlier")):
        out.append(_single(f"mode-{mode}", "mode", 4, 2, 128, 300, 512,
                           [0, 150, -1], 16, seed=400 + i, mode=mode))
    # ---- batched (BATCH=1 instantiations) -----------------------------------
    pos = (0, 37, 127)
    out.append(Spec("batched-B3", "batched",
                    dict(qpk=4, n_kv=2, hs=128, pos=list(pos),
                         slot=[2, 0, 1], max_seq=128, seed=500,
                         probes=[pick_probes(p + 1, [0, 15, 16, p - 1, p])
                                 for p in pos]),
                    8, extra=dict(n_batch=3)))
    out.append(Spec("batched-B1", "batched",
                    dict(qpk=4, n_kv=2, hs=128, pos=[82], slot=[2],
                         max_seq=128, seed=501,
                         probes=[pick_probes(83, [0, 15, 16, 81, 82])]),
                    8, extra=dict(n_batch=1)))
    # ---- implicit dispatch: max_seq=8192 takes the split path unforced -----
    out.append(_single("implicit-maxseq8192", "implicit", 4, 2, 128, 300,
                       8192, [0, 15, 16, -1], 32, paths=("split",),
                       force_split=False, seed=600))
    return out


SPECS = _specs()
CASES = [(s, path, kv8) for s in SPECS for path in s.paths
         for kv8 in (False, True)]
CASE_IDS = [f"{s.name}-{path}-{'fp8' if kv8 else 'bf16'}"
            for s, path, kv8 in CASES]


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def _dev(t):
    return None if t is None else t.to(DEV)


def _i32(v):
    return torch.tensor(v, device=DEV, dtype=torch.int32)


def launch(ops, case, n_chunks, force_split, n_batch):
    """Run attn_decode on device copies; returns (out, tail ok, pools before
    and after, qkv unchanged, split partials written)."""
    beff = max(n_batch, 1)
    n = beff * case.n_head * case.hs
    buf = torch.full((n + GUARD,), 12352.0, device=DEV, dtype=torch.bfloat16)
    tail = buf[n:].clone()
    qkv = case.qkv.to(DEV).reshape(-1).contiguous()
    qkv0 = qkv.clone()
    pools = [_dev(t) for t in (case.kpool, case.vpool, case.kscale,
                               case.vscale)]
    before = [None if t is None else t.clone() for t in pools]
    # partials start as NaN: a chunk slot read before it was written shows
    part_o = torch.full((n * n_chunks,), float("nan"), device=DEV)
    part_ml = torch.full((beff * case.n_head * n_chunks * 2,), float("nan"),
                         device=DEV)
    ops.attn_decode(buf[:n], part_o, part_ml, qkv, pools[0], pools[1],
                    case.cos.to(DEV), case.sin.to(DEV), _i32(case.pos),
                    _i32(case.slot), case.layer, n_chunks, case.scale,
                    n_batch=n_batch, kscale=pools[2], vscale=pools[3],
                    force_split=int(force_split))
    torch.cuda.synchronize()
    return (buf[:n].clone(), torch.equal(buf[n:], tail), before, pools,
            torch.equal(qkv, qkv0), not bool(torch.isnan(part_ml).all()))


def check_append(case, ref, before, after):
    """(2) the appended row and (3) nothing else written."""
    B = len(case.pos)
    k_row = ref.k_row if case.batched else ref.k_row[None]
    v_row = ref.v_row if case.batched else ref.v_row[None]
    for b in range(B):
        idx = (case.slot[b], case.layer, slice(None), case.pos[b])
        gk, gv = after[0][idx].cpu(), after[1][idx].cpu()
        if not case.kv8:
            d = bf16_ulp_distance(gk, k_row[b].to(torch.bfloat16))
            assert int(d.max()) <= 1, f"appended K off by {int(d.max())} ulp"
            assert torch.equal(gv, v_row[b].to(torch.bfloat16)), \
                "appended V is not the raw v"
            continue
        for name, got, tbl, src in (("K", gk, after[2], k_row[b]),
                                    ("V", gv, after[3], v_row[b])):
            sc = tbl[idx].cpu()
            want = src.abs().amax(-1).clamp_min(1e-12) / 448.0
            assert torch.allclose(sc.double(), want, rtol=1e-6, atol=0), \
                f"{name} scale {sc.tolist()} != {want.tolist()}"
            deq = fp8_decode(got).double() * sc.double()[:, None]
            tol = 2.0 ** -4 * src.abs() + sc.double()[:, None] * 2.0 ** -10
            assert bool(((deq - src).abs() <= tol).all()), \
                f"appended fp8 {name} row outside the e4m3 half-ulp"
    for t0, t1 in zip(before, after):
        if t0 is None:
            continue
        t1 = t1.clone()
        for b in range(B):
            idx = (case.slot[b], case.layer, slice(None), case.pos[b])
            t1[idx] = t0[idx]
        assert torch.equal(t1, t0), "a row other than [slot, layer, :, pos] " \
                                    "was written"


def run_and_check(ops, spec, path, kv8):
    case = make_case(kv8=kv8, **spec.kw)
    ref = case.reference()
    assert case.probes_ok(ref), \
        f"precondition: probe weights {case.probe_weights(ref)}"
    n_batch = spec.extra.get("n_batch", 0)
    out, tail_ok, before, after, qkv_ok, split_ran = launch(
        ops, case, spec.n_chunks, path == "split" and spec.force_split,
        n_batch)
    # the split-S kernel leaves its (m, l) partials behind, the block-local
    # kernel never touches them: the case ran on the path it names
    assert split_ran == (path == "split"), "wrong kernel dispatched"
    got = out.cpu().reshape(ref.out.shape)
    ratio = attn_error_ratio(got, ref.out, ref.A)
    print(f"ATTN_RATIO {spec.family} {path} {'fp8' if kv8 else 'bf16'} "
          f"{spec.name} {ratio:.4f}")
    assert attn_error_ok(got, ref.out, ref.A), \
        f"|got-ref|/bound = {ratio:.3f} (must be <= 1)"
    check_append(case, ref, before, after)
    assert tail_ok, "out written past n_batch * n_head * hs"
    assert qkv_ok, "the raw qkv buffer was modified"
    return case, ref, got


@pytest.mark.parametrize("spec,path,kv8", CASES, ids=CASE_IDS)
def test_attn_decode_matrix(ops, spec, path, kv8):
    case, ref, got = run_and_check(ops, spec, path, kv8)
    if spec.family != "batched":
        return
    # each sample also matches the single-sample reference of its own slot
    from attn_reference import attn_decode_reference

    for b in range(len(case.pos)):
        one = attn_decode_reference(
            case.qkv[b], case.kpool, case.vpool, case.cos, case.sin,
            case.pos[b], case.slot[b], case.layer, case.scale, case.kscale,
            case.vscale)
        assert attn_error_ok(got[b], one.out, one.A), f"sample {b}"


@pytest.mark.parametrize("n_chunks", [6, 260])
def test_attn_decode_rejects_bad_n_chunks(ops, n_chunks):
    """n_chunks must be a multiple of 4 (block-shared q staging) and at
    most 256 (the combine's weight registers); the binding refuses anything
    else before any launch."""
    case = make_case(qpk=4, n_kv=2, hs=128, pos=82, max_seq=128,
                     probes=[0, 82], seed=700)
    with pytest.raises(RuntimeError, match="n_chunks"):
        launch(ops, case, n_chunks, True, 0)


def test_attn_decode_rejected_call_launches_nothing(ops):
    case = make_case(qpk=4, n_kv=2, hs=128, pos=82, max_seq=128,
                     probes=[0, 82], seed=701)
    n = case.n_head * case.hs
    out = torch.full((n,), 12352.0, device=DEV, dtype=torch.bfloat16)
    kpool, vpool = case.kpool.to(DEV), case.vpool.to(DEV)
    part_o = torch.zeros(n * 260, device=DEV)
    part_ml = torch.zeros(case.n_head * 260 * 2, device=DEV)
    with pytest.raises(RuntimeError, match="n_chunks"):
        ops.attn_decode(out, part_o, part_ml, case.qkv.to(DEV).reshape(-1),
                        kpool, vpool, case.cos.to(DEV), case.sin.to(DEV),
                        _i32(case.pos), _i32(case.slot), case.layer, 260,
                        case.scale, force_split=1)
    torch.cuda.synchronize()
    assert bool((out == 12352.0).all())
    assert torch.equal(kpool.cpu(), case.kpool)
    assert torch.equal(vpool.cpu(), case.vpool)
