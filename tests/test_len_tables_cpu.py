"""The length tables a batch run builds on the host and uploads in front of its pipeline (csrc/host/len_tables.cpp, through
stn_dbg_len_tables — no device): against numpy restatements of what the kernels they replace write.  tests/test_gpu_len_tables.py holds the
same tables against the kernels themselves.

Cases (tests/len_tables_ref.py): B in {1, 2, 3, 128, 1024}; all lengths equal (every comparison of the pairing a tie), strictly descending,
one length of 1, many ties, odd B; the estimator's rows exact and rounded up to a bucket of 64 (dead rows); both trim forms and the scaled
lengths; for the trim forms a row length T on each side of the 10 % bar Engine::vocoder_rows holds the batch to (the builder does not decide
the form: it must be right on both sides) and utterances that reach the end of the row (l6 + 2rf > T, l6 + rf > T)."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.binding import LEN_VO_2RF, LEN_VO_NONE, LEN_VO_SCALED, LEN_VO_TAIL

from len_tables_ref import bucket_up, cases, hs_pairs, row_map, vo_extents

CCF, RF = 6, 57
CASES = cases()


@pytest.mark.parametrize("name,llen", CASES, ids=[c[0] for c in CASES])
def test_estimator_maps_and_pairs(name, llen):
    tot = int(llen.sum())
    for rows in (tot, bucket_up(tot, 64), bucket_up(tot, 64) + 64):
        t = binding.len_tables(llen, ve_rows=rows, with_pairs=True)
        off, row_b = row_map(llen, rows)
        assert np.array_equal(t["llen"], llen)
        assert np.array_equal(t["ve_off"], off) and np.array_equal(t["ve_row_b"], row_b[:rows])
        assert np.array_equal(t["pairs"], hs_pairs(llen))
        assert "vo_n" not in t
        p = t["pairs"][:2 * ((len(llen) + 1) // 2)]
        assert sorted(int(v) for v in p if v >= 0) == list(range(len(llen)))  # every utterance exactly once
    t = binding.len_tables(llen, ve_rows=tot, with_pairs=False)
    assert "pairs" not in t and np.array_equal(t["ve_off"], row_map(llen, tot)[0])
    t = binding.len_tables(llen)
    assert set(t) == {"llen", "total"} and t["total"] % 4 == 0


@pytest.mark.parametrize("form", (LEN_VO_2RF, LEN_VO_TAIL, LEN_VO_SCALED))
@pytest.mark.parametrize("name,llen", CASES, ids=[c[0] for c in CASES])
def test_vocoder_extents(name, llen, form):
    L = int(llen.max())
    for T in (L * CCF, (L + 1) * CCF, (L + 30) * CCF, (L + 200) * CCF):  # the longest reaches the end of its row; ...; nearly all of it padding
        t = binding.len_tables(llen, vo_form=form, ccf=CCF, T=T, rf=RF)
        n, valid, off = vo_extents(llen, form, CCF, T, RF)
        assert np.array_equal(t["vo_n"], n) and np.array_equal(t["vo_valid"], valid) and np.array_equal(t["vo_off"], off), (name, T)
        assert np.all(t["vo_valid"] <= t["vo_n"]) and (form == LEN_VO_SCALED or np.all(t["vo_n"] <= T))


def test_both_sides_of_the_ten_percent_bar():
    """Engine::vocoder_rows trims when the packed rows are at most 90 % of B * T: tables for a batch just below and just above that"""
    llen = np.array([60, 60, 60, 50], np.int32)
    for T in (60 * CCF, 75 * CCF):
        for form in (LEN_VO_2RF, LEN_VO_TAIL):
            t = binding.len_tables(llen, vo_form=form, ccf=CCF, T=T, rf=RF)
            n, valid, off = vo_extents(llen, form, CCF, T, RF)
            assert np.array_equal(t["vo_n"], n) and np.array_equal(t["vo_valid"], valid) and np.array_equal(t["vo_off"], off)
    below = vo_extents(llen, LEN_VO_TAIL, CCF, 75 * CCF, RF)[0].sum() * 10 <= 4 * 75 * CCF * 9
    above = vo_extents(llen, LEN_VO_TAIL, CCF, 60 * CCF, RF)[0].sum() * 10 <= 4 * 60 * CCF * 9
    assert below and not above  # the two batches do lie on either side


def test_everything_at_once_and_the_layout():
    llen = np.array([9, 3, 9, 1, 7], np.int32)
    t = binding.len_tables(llen, ve_rows=64, with_pairs=True, vo_form=LEN_VO_TAIL, ccf=CCF, T=10 * CCF, rf=4)
    assert np.array_equal(t["ve_row_b"][:29], np.repeat(np.arange(5), llen)) and not t["ve_row_b"][29:].any()
    assert list(t["pairs"]) == [2, 3, 0, 1, 4, -1, 0]
    assert list(t["vo_n"]) == [58, 22, 58, 10, 46] and list(t["vo_valid"]) == [58, 22, 58, 10, 46]
    assert t["total"] == (2 + 5 + 6 + 64 + 7 + 5 + 5 + 6 + 3) // 4 * 4


def test_bad_arguments():
    with pytest.raises(binding.StnError):
        binding.len_tables(np.array([5, 6], np.int32), ve_rows=10)  # fewer rows than the lengths sum to
    with pytest.raises(binding.StnError):
        binding.len_tables(np.array([5, 6], np.int32), with_pairs=True)  # pairs without packed rows
    with pytest.raises(binding.StnError):
        binding.len_tables(np.array([5, -1], np.int32))
    with pytest.raises(binding.StnError):
        binding.len_tables(np.array([5], np.int32), vo_form=4)
    with pytest.raises(binding.StnError):
        binding.len_tables(np.ones(1025, np.int32))
