"""GPU: the fused sampler (launch_sample and the sample_* kernels) draw for
draw against the CPU reference of sampler_reference.py.

The radix select works on integer codes and the RNG is an integer hash, so
the reference says exactly which token every call must return, up to the
fp32 rounding of the score (eps) and of the top-p mass (delta); both are
derived in sampler_reference's docstring and none is set here.  A case runs
as ONE batched call of n rows of identical logits and distinct pos (the
32-block geometry), and its first 64 draws again through the one-row path
(128 blocks); both must agree with the reference.  Every threshold case
also has to DISAGREE with deliberately wrong references (threshold one code
off either way, pos and slot swapped, top-p mass not restricted to the
top-k set), or the case would prove nothing.

Each case prints its tally; profiles/sampler_error_margins.md keeps the
figures of one run.
"""

import numpy as np
import pytest
import torch

import sampler_reference as R
from sampler_reference import (BATCH_MODES, BATCH_T, SHAPE_CASES,
                               SINGLE_DRAWS, THRESHOLD_CASES, TIE_CASES,
                               batch_rows, case_keys, case_logits,
                               case_reference, check_draws, draw_many,
                               final_threshold, inv_temp_f32,
                               perturbed_winners, tie_logits)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROW = R.SCRATCH_PER_ROW


@pytest.fixture(scope="module")
def ops():
    from mdi_llm_amd.ops import require_hip_ops

    return require_hip_ops()


def _i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(DEV)


def new_scratch(rows=1):
    return torch.zeros(rows * ROW, device=DEV, dtype=torch.int32)


def sample_rows(ops, logits, T, k, p, seed, pos, slot, noise=True,
                scratch=None, pos_bias=0):
    """One batched call: row b of logits [B, V] under key (pos[b], slot[b]);
    slot None leaves the kernel's default.  Returns the B tokens."""
    B = logits.shape[0]
    assert B > 1 and logits.is_contiguous()
    scratch = new_scratch(B) if scratch is None else scratch
    out = torch.full((B,), -7, device=DEV, dtype=torch.int32)
    ops.sample(out, logits, scratch, T, k, noise, seed, pos=_i32(pos),
               slot=None if slot is None else _i32(slot), n_batch=B,
               top_p=p, pos_bias=pos_bias)
    return out.cpu().numpy().astype(np.int64)


def sample_singles(ops, logits, T, k, p, seed, pos, slot, noise=True,
                   scratch=None, pos_bias=0):
    """One one-row call per key, all on the same scratch.  logits is [V] or
    [n, V].  Returns the n tokens."""
    pos, slot = _i32(pos), _i32(slot)
    n = pos.numel()
    scratch = new_scratch() if scratch is None else scratch
    out = torch.full((n,), -7, device=DEV, dtype=torch.int32)
    for j in range(n):
        row = logits if logits.dim() == 1 else logits[j]
        ops.sample(out[j:j + 1], row, scratch, T, k, noise, seed,
                   pos=pos[j:j + 1], slot=slot[j:j + 1], top_p=p,
                   pos_bias=pos_bias)
    return out.cpu().numpy().astype(np.int64)


def assert_clean(scratch, rows=1):
    s = scratch.view(rows, ROW)[:, :R.SCRATCH_CLEANED]
    assert int(s.count_nonzero()) == 0, "scratch [0, 518) is not clean"


def run_case(ops, case):
    """(tokens of the batched call, tokens of the first draws one by one)"""
    lg = case_logits(case).to(DEV)
    pos, slot = case_keys(case)
    m = min(case.n, SINGLE_DRAWS)
    scr1 = new_scratch()
    single = sample_singles(ops, lg, case.T, case.k, case.p, case.seed,
                            pos[:m], slot[:m], scratch=scr1)
    assert_clean(scr1)
    if case.n == 1:
        return single, single
    scrB = new_scratch(case.n)
    rows = lg.unsqueeze(0).expand(case.n, case.V).contiguous()
    batched = sample_rows(ops, rows, case.T, case.k, case.p, case.seed, pos,
                          slot, scratch=scrB)
    assert_clean(scrB, case.n)
    return batched, single


def hold_to_reference(ops, case):
    t, margin, delta, ref = case_reference(case)
    # preconditions of the case, on the reference alone
    assert int(ref.decisive.sum()) >= (1 - R.MAX_NONDECISIVE) * case.n
    assert margin >= delta
    batched, single = run_case(ops, case)
    dec_b, n_b, msg = check_draws(ref, batched)
    assert not msg, f"{case.id} batched: {msg}"
    dec_s, n_s, msg = check_draws(ref.head(single.shape[0]), single)
    assert not msg, f"{case.id} single: {msg}"
    print(f"{case.id}: kept {ref.kept.size}, batched {dec_b}/{n_b} decisive "
          f"draws exact, single {dec_s}/{n_s}, min gap {ref.gap.min():.3g}, "
          f"max eps {ref.eps.max():.3g}, margin {margin:.3g}, "
          f"delta {delta:.3g}")
    return batched


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(THRESHOLD_CASES))
def test_threshold_case(ops, name):
    """Exact winners on every decisive draw, and disagreement with every
    perturbed reference of the case."""
    case = THRESHOLD_CASES[name]
    got = hold_to_reference(ops, case)
    for tooth in case.teeth:
        wrong = perturbed_winners(case, tooth)
        assert (got != wrong).any(), (
            f"{name}: the kernel agrees on every draw with the reference "
            f"perturbed by '{tooth}': the case has no teeth")


@pytest.mark.parametrize("name", list(SHAPE_CASES))
def test_vocabulary_shape(ops, name):
    """V = 1, under one wave, no multiple of the grid stride, one past it,
    the workload's 128256; top_k above V is inactive."""
    hold_to_reference(ops, SHAPE_CASES[name])


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TIE_CASES))
def test_greedy_tie_takes_lowest_index(ops, name):
    """Equal maxima, noise off, temperature 0: the lowest index, through
    the one-row launch (128 blocks) and as row 1 of a batched one (32
    blocks).  Before the tie-rule fix the cross-wave atomicMax took the
    higher index whenever the maxima sat in different waves: (5, 70) gave
    70, (300, 9000, 33000) gave 33000, and (0, 8192) gave 8192 from the
    one-row launch but 0 from the batched one, where the two indices share
    a thread."""
    V, idx = TIE_CASES[name]
    lg = tie_logits(name).to(DEV)
    want = min(idx)
    assert int(torch.argmax(lg.float())) == want
    single = sample_singles(ops, lg, 0.0, 0, 1.0, 1, [0], [0], noise=False)
    other = tie_logits("same_wave").to(DEV).roll(1234)
    rows = torch.stack([other, lg]).contiguous()
    batched = sample_rows(ops, rows, 0.0, 0, 1.0, 1, [0, 0], [0, 1],
                          noise=False)
    print(f"{name}: tied at {idx}: single {int(single[0])}, "
          f"batched row {int(batched[1])}")
    assert int(single[0]) == want
    assert int(batched[1]) == want
    assert int(batched[0]) == int(torch.argmax(other.float()))


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(BATCH_MODES))
@pytest.mark.parametrize("B", [2, 5, 16])
def test_batched_equals_single(ops, B, mode):
    """Distinct logits, pos and slot per row: row b is the one-row call with
    that row's logits and key, and both are the reference's winner.  With
    no slot given the batched key of row b is b."""
    k, p = BATCH_MODES[mode]
    rows, pos, slot = batch_rows(B)
    rows_d = rows.to(DEV)
    for use_slot in (slot, None):
        keyed = slot if use_slot is not None else np.arange(B)
        batched = sample_rows(ops, rows_d, BATCH_T, k, p, 21, pos, use_slot)
        single = sample_singles(ops, rows_d, BATCH_T, k, p, 21, pos, keyed)
        for b in range(B):
            t, margin, delta = final_threshold(rows[b], BATCH_T, k, p)
            assert margin >= delta
            ref = draw_many(rows[b], t, inv_temp_f32(BATCH_T), True, 21,
                            [pos[b]], [keyed[b]])
            assert ref.decisive.all()
            assert int(batched[b]) == int(ref.winner[0]), (b, mode)
            assert int(single[b]) == int(ref.winner[0]), (b, mode)


# ---------------------------------------------------------------------------
def _sequence(ops, lg, seed, pos0, slot, pos_bias=0, n=32):
    rows = lg.unsqueeze(0).expand(n, lg.numel()).contiguous()
    return sample_rows(ops, rows, 1.0, 0, 1.0, seed, pos0 + np.arange(n),
                       np.full(n, slot), pos_bias=pos_bias)


def test_key_plumbing(ops):
    """pos_bias adds to pos; seed, pos and slot each change the sequence."""
    case = SHAPE_CASES["V1000"]
    lg = case_logits(case).to(DEV)
    base = _sequence(ops, lg, 7, 40, 2)
    ref = draw_many(case_logits(case), 0, inv_temp_f32(1.0), True, 7,
                    40 + np.arange(32), np.full(32, 2))
    assert not check_draws(ref, base)[2]
    assert len(set(base.tolist())) > 8
    shifted = _sequence(ops, lg, 7, 39, 2, pos_bias=1)
    assert (shifted == base).all()
    one = sample_singles(ops, lg, 1.0, 0, 1.0, 7, 39 + np.arange(4),
                         np.full(4, 2), pos_bias=1)
    assert (one == base[:4]).all()
    for name, other in (("seed", _sequence(ops, lg, 8, 40, 2)),
                        ("pos", _sequence(ops, lg, 7, 140, 2)),
                        ("slot", _sequence(ops, lg, 7, 40, 3))):
        assert (other != base).any(), f"{name} does not reach the RNG key"


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(BATCH_MODES))
def test_scratch_is_left_clean_and_reusable(ops, mode):
    """After a call entries [0, 518) of every row's scratch are zero, and a
    second identical call on the same scratch returns the same tokens."""
    k, p = BATCH_MODES[mode]
    rows, pos, slot = batch_rows(5)
    rows_d = rows.to(DEV)
    scr = new_scratch(5)
    a = sample_rows(ops, rows_d, BATCH_T, k, p, 3, pos, slot, scratch=scr)
    assert_clean(scr, 5)
    b = sample_rows(ops, rows_d, BATCH_T, k, p, 3, pos, slot, scratch=scr)
    assert_clean(scr, 5)
    assert (a == b).all()
    scr1 = new_scratch()
    c = sample_singles(ops, rows_d[0], BATCH_T, k, p, 3, pos[:1], slot[:1],
                       scratch=scr1)
    assert_clean(scr1)
    d = sample_singles(ops, rows_d[0], BATCH_T, k, p, 3, pos[:1], slot[:1],
                       scratch=scr1)
    assert_clean(scr1)
    assert int(c[0]) == int(d[0]) == int(a[0])


def test_scratch_carries_nothing_between_modes(ops):
    """'k and p' and then 'none' on the same scratch: what a fresh scratch
    returns, one row and batched."""
    rows, pos, slot = batch_rows(5)
    rows_d = rows.to(DEV)
    k, p = BATCH_MODES["k_and_p"]
    fresh = sample_rows(ops, rows_d, BATCH_T, 0, 1.0, 3, pos, slot)
    scr = new_scratch(5)
    sample_rows(ops, rows_d, BATCH_T, k, p, 3, pos, slot, scratch=scr)
    again = sample_rows(ops, rows_d, BATCH_T, 0, 1.0, 3, pos, slot,
                        scratch=scr)
    assert (again == fresh).all()
    scr1 = new_scratch()
    sample_singles(ops, rows_d[2], BATCH_T, k, p, 3, pos[2:3], slot[2:3],
                   scratch=scr1)
    one = sample_singles(ops, rows_d[2], BATCH_T, 0, 1.0, 3, pos[2:3],
                         slot[2:3], scratch=scr1)
    assert int(one[0]) == int(fresh[2])
