"""The context model and its committed sequences, without a device (tests/context_model.py): the coverage the sequences
promise is counted, every sequence runs on the model with the oracle alone, and the model obeys the identities the header
promises — where a mistake in the model shows before a GPU is involved."""
import ctypes as C
import time

import numpy as np
import pytest

import context_model as M
from ray_tracer_webgl_amd import abi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dry_codes():
    """(test, sequence index) -> the return code the model predicts for every step"""
    return {(name, k): M.run_model(seq, M.DryRenderer())[1] for name, seqs in M.SEQUENCES.items() for k, seq in enumerate(seqs)}


def accepted_runs(dry_codes):
    """every sequence as the list of its accepted calls, checks left out: what stands "directly" before and after what"""
    for (name, k), codes in dry_codes.items():
        seq = M.SEQUENCES[name][k]
        yield name, seq, codes


def test_no_sequence_holds_an_operation_outside_the_table():
    for name, seqs in M.SEQUENCES.items():
        for seq in seqs:
            for op, v in seq:
                assert (op, v) == M.CHECK or (op in M.OPS and 0 <= v < M.OPS[op].variants), (name, op, v)


def test_every_ordered_pair_of_configuration_operations_is_followed_by_work_and_a_check(dry_codes):
    required = {(x, y) for x in M.CONFIG for y in M.CONFIG}
    covered = set()
    for name, seq, codes in accepted_runs(dry_codes):
        for i in range(len(seq) - 3):
            (x, _), (y, _), (w, _), c = seq[i:i + 4]
            if x in M.CONFIG and y in M.CONFIG and w in M.WORKS and c == M.CHECK and codes[i:i + 3] == [M.OK] * 3:
                covered.add((x, y))
    print("pair coverage: %d / %d" % (len(covered & required), len(required)))
    assert len(M.CONFIG) == 19 and covered >= required, sorted(required - covered)


def test_every_configuration_operation_stands_directly_before_and_after_frames_adaptive_tune_and_a_replayed_capture(dry_codes):
    """(a check between two calls only reads: "directly" looks through it)"""
    after, before = set(), set()
    for name, seq, codes in accepted_runs(dry_codes):
        calls = [(op, rc) for (op, v), rc in zip(seq, codes) if (op, v) != M.CHECK]
        for (a, ra), (b, rb) in zip(calls, calls[1:]):
            if ra == M.OK and rb == M.OK:
                if a in M.NEIGHBOURS and b in M.CONFIG:
                    after.add((a, b))
                if b in M.NEIGHBOURS and a in M.CONFIG:
                    before.add((a, b))
    want_after = {(n, c) for n in M.NEIGHBOURS for c in M.CONFIG}
    want_before = {(c, n) for n in M.NEIGHBOURS for c in M.CONFIG}
    assert after >= want_after, sorted(want_after - after)
    assert before >= want_before, sorted(want_before - before)


def test_every_variant_of_every_operation_is_used_and_tests_are_named_after_their_leading_operation():
    used = {s for seqs in M.SEQUENCES.values() for seq in seqs for s in seq}
    for name, op in M.OPS.items():
        assert all((name, v) in used for v in range(op.variants)), name
    assert set(M.SEQUENCES) == set(M.CONFIG) | {"refusals"}
    for x in M.CONFIG:
        for seq in M.SEQUENCES[x]:
            body = seq[len(M.PROLOGUE):]
            triples = [i for i in range(len(body) - 3) if body[i][0] == x and body[i + 1][0] in M.CONFIG
                       and body[i + 2][0] in M.WORKS and body[i + 3] == M.CHECK]
            assert len(triples) >= 9, x


def test_the_refusals_are_the_documented_ones(dry_codes):
    codes = dry_codes[("refusals", 0)]
    assert len(codes) == len(M.REFUSED)
    for i, (got, want) in enumerate(zip(codes, M.REFUSED)):
        assert got == (M.OK if want is None else want), (i, M.REFUSALS[i], got, want)
    assert sum(c is not None for c in M.REFUSED) == 12
    for (name, k), codes in dry_codes.items():   # ... and nowhere else is a call refused
        if name != "refusals":
            assert all(c == M.OK for c in codes), (name, k)


def test_every_sequence_runs_on_the_model_with_the_oracle_alone(ora, dry_codes):
    t0 = time.time()
    for name, seqs in M.SEQUENCES.items():
        for k, seq in enumerate(seqs):
            m, codes = M.run_model(seq, M.OracleRenderer())
            assert codes == dry_codes[(name, k)], (name, k)   # the dry model chose the variants: it must predict the same codes
    print("model runs of all sequences: %.1f s" % (time.time() - t0))


def test_the_scenes_get_the_structures_the_sequences_count_on():
    lib = M.scenes._lib()
    for name in M.SCENES:
        ptr, n, keep = abi.spheres_as_ctypes(M.scene(name))
        counts = (C.c_uint32 * 8)()
        rc = lib.pt_build_grid(ptr, n, counts, None, None, None, None, 0, None, 0, None, 0)
        assert (rc == abi.PT_OK) == M.HAS_GRID[name], (name, rc)
        if name == "flat130":
            assert n == 130 and counts[1] == 1 and counts[0] > 1 and counts[2] > 1   # one layer of cells
        if name == "random40":
            assert n == 40 and counts[1] > 1


# ------------------------------------------------------------------------------------------------ the header's identities
def _model(ora, scene="default", size=M.SIZES[1]):
    m = M.start(M.OracleRenderer(), size)
    m.set_spheres(scene)
    m.reserve(3)
    return m


@pytest.mark.parametrize("estimate", [False, True])
def test_passes_in_one_call_equal_the_same_passes_split_over_calls(ora, estimate):
    one, split = _model(ora), _model(ora)
    for m in (one, split):
        m.set_estimate(estimate)
    assert one.render_passes(3) == M.OK
    assert split.render_passes(1) == M.OK
    p = split.params.copy()
    p.first_pass += 1
    split.set_params(p)
    assert split.render_passes(2) == M.OK
    assert np.array_equal(bits(one.accum), bits(split.accum)) and one.segments == split.segments and one.total_spp == 6
    if estimate:
        assert np.array_equal(bits(one.err), bits(split.err))
        until = _model(ora)
        until.set_estimate(True)
        assert until.render_to_target(2, 3, False) == M.OK and until.params.first_pass == 3
        assert np.array_equal(bits(one.accum), bits(until.accum)) and np.array_equal(bits(one.err), bits(until.err))


def test_band_pieces_reassemble_to_the_whole_frame(ora):
    lib = M.scenes._lib()
    whole = _model(ora, "random40")
    assert whole.render_passes(2) == M.OK
    for rows, _, count in M.BANDS[1:]:
        frame = np.full_like(whole.accum, np.nan)
        seg = 0
        for index in range(count):
            m = _model(ora, "random40")
            p = m.params.copy()
            p.band_rows, p.band_index, p.band_count = rows, index, count
            m.set_params(p)
            assert m.render_passes(2) == M.OK and m.rows == lib.pt_local_rows(m.h, rows, index, count)
            for l in range(m.rows):
                frame[lib.pt_band_row(rows, index, count, l)] = m.accum[l]
            seg += m.segments
        assert np.array_equal(bits(frame), bits(whole.accum)) and seg == whole.segments


def test_a_checkpoint_followed_by_a_resume_equals_the_uninterrupted_run(ora):
    whole, first, second = _model(ora), _model(ora), _model(ora)
    assert whole.render_passes(3) == M.OK
    assert first.render_passes(1) == M.OK
    p = second.params.copy()
    p.first_pass = 1
    second.set_params(p)
    assert second.load_accum(first.accum) == M.OK and second.total_spp == 2
    assert second.render_passes(2) == M.OK
    assert np.array_equal(bits(second.accum), bits(whole.accum))
    assert second.load_accum(np.zeros((3, 3, 4), np.float32)) == M.INVALID   # another size: refused, nothing changed
    assert np.array_equal(bits(second.accum), bits(whole.accum))
