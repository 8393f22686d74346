// len_tables.hpp — everything the replayed pipeline derives from the utterances' latent lengths alone, built on the host: the estimator's
// packed-row map, the head-split cross-attention's pairing, the vocoder's extents and its packed-row offsets.  The host holds the lengths
// before the pipeline starts (Engine::batch_run), so these tables ride up in the one copy that carries the lengths and the noise seed, and
// the single-workgroup kernels that used to compute them (row_map_kernel, hs_pairs_kernel, trim_len_kernel, scale_len_kernel) leave the
// dependent chain.  Every table holds exactly the integers its kernel writes (tests/test_len_tables_cpu.py, tests/test_gpu_len_tables.py).
#pragma once
#include <cstdint>

namespace stn {

enum LenVoForm : int {
    LEN_VO_NONE = 0,    // the dense vocoder: no vocoder tables
    LEN_VO_2RF = 1,     // trim_len_kernel, tail_form = 0
    LEN_VO_TAIL = 2,    // trim_len_kernel, tail_form = 1
    LEN_VO_SCALED = 3,  // the length-aware vocoder: scale_len_kernel (n = valid = len * ccf)
};

// the block's layout in 32-bit words; a table that is not built has offset -1
struct LenTables {
    int seed = 0;       // 2 words: the 64-bit noise seed (the caller's)
    int llen = 2;       // [B] the lengths themselves
    int ve_off = -1;    // [B + 1]    row_map_kernel's row_off          (ve_rows > 0)
    int ve_row_b = -1;  // [ve_rows]  row_map_kernel's row_b, dead rows (those behind sum len) = 0
    int pairs = -1;     // [B + 2]    hs_pairs_kernel's table in its first 2 * ceil(B / 2) words, the rest 0   (with_pairs)
    int vo_n = -1;      // [B]        rows each utterance is decoded on                         (vo_form != LEN_VO_NONE)
    int vo_valid = -1;  // [B]        rows of those that are its own output
    int vo_off = -1;    // [B + 1]    row_map_kernel's row_off over vo_n
    int total = 0;      // words
};

// ve_rows: the estimator's packed row count with its dead rows (0: padded rows, no map); sizes follow from B, ve_rows and the two switches alone
LenTables len_tables_layout(int B, int ve_rows, bool with_pairs, int vo_form);
// fills out[t.llen ..] .. out[t.total) (the seed words are the caller's).  ccf: vocoder frames per latent frame; T: frames of a padded row;
// rf: the vocoder's receptive field.  ve_rows >= sum llen.
void len_tables_build(const LenTables& t, const int* llen, int B, int ve_rows, bool with_pairs, int vo_form, int ccf, int T, int rf, int32_t* out);

}  // namespace stn
