"""The host-built length tables (csrc/host/len_tables.cpp) against what the kernels they replace in the batch pipeline write on the device:
row_map_kernel (offsets, row -> sequence, dead rows), hs_pairs_kernel (the head-split cross-attention's pairing) and trim_len_kernel (both
forms), each through stn_op_layout.  Same cases as tests/test_len_tables_cpu.py; integers, so equality."""
import numpy as np
import pytest

from supertonic_amd import binding
from supertonic_amd.binding import LAYOUT_HS_PAIRS, LAYOUT_ROW_MAP, LAYOUT_TRIM_LEN, LEN_VO_2RF, LEN_VO_TAIL

from len_tables_ref import bucket_up, cases

pytestmark = pytest.mark.gpu

CCF, RF = 6, 57
CASES = cases()


@pytest.fixture(scope="module")
def eng():
    return binding.Engine(0, "bf16")


@pytest.mark.parametrize("name,llen", CASES, ids=[c[0] for c in CASES])
def test_tables_equal_the_kernels(eng, name, llen):
    B, tot = len(llen), int(llen.sum())
    rows = bucket_up(tot, 64) + (64 if B % 2 else 0)  # dead rows: a part of a bucket, or that and a whole one
    T = (int(llen.max()) + 25) * CCF
    for form in (LEN_VO_2RF, LEN_VO_TAIL):
        t = binding.len_tables(llen, ve_rows=rows, with_pairs=True, vo_form=form, ccf=CCF, T=T, rf=RF)
        io = eng.op_layout(LAYOUT_ROW_MAP, [B, rows, 1], length=llen, iout=np.full(B + 1 + rows, -7, np.int32))[2]
        assert np.array_equal(io[:B + 1], t["ve_off"]) and np.array_equal(io[B + 1:], t["ve_row_b"])
        G2 = 2 * ((B + 1) // 2)
        io = eng.op_layout(LAYOUT_HS_PAIRS, [B], length=llen, iout=np.full(G2, -7, np.int32))[2]
        assert np.array_equal(io, t["pairs"][:G2])
        io = eng.op_layout(LAYOUT_TRIM_LEN, [B, CCF, T, RF, int(form == LEN_VO_TAIL)], length=llen, iout=np.full(2 * B, -7, np.int32))[2]
        assert np.array_equal(io[:B], t["vo_n"]) and np.array_equal(io[B:], t["vo_valid"])
        io = eng.op_layout(LAYOUT_ROW_MAP, [B, 0, 0], length=t["vo_n"], iout=np.full(B + 1, -7, np.int32))[2]
        assert np.array_equal(io, t["vo_off"])
