// join_plan.hpp — the plan of a joined fetch (include/stn.h, "join"): where every member's segment lands in its
// programme's row, the programmes' lengths and their durations.  Host arithmetic only: the engine's output stage, stn_join_plan and
// the hosts that size buffers share it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/stn.h"

namespace stn {

struct JoinPlan {
    int G = 0, B = 0;
    int64_t W_join = 0;
    std::vector<int32_t> first;                        // [G] first member (batch row) of each programme
    std::vector<int64_t> seg_len, seg_dst;             // [B]
    std::vector<int64_t> prog_len;                     // [G]
    std::vector<float> prog_dur;                       // [G]
    // [B] each, or all three empty: with silence trimming on the segment's first source sample and the samples
    // faded at its head and its tail; the engine's output stage fills them, join_plan leaves them empty
    std::vector<int64_t> seg_src;
    std::vector<int32_t> seg_fin, seg_fout;
    // with the pause limit a member is several pieces of its row, laid end to end from seg_dst: member i's are
    // [piece_first[i], piece_first[i + 1]) (B + 1 entries), piece_dst counted in the programme's row.  All empty: a member is one piece
    // and seg_* describe it.  seg_len stays the member's delivered length.  Filled by the engine's output stage only.
    std::vector<int32_t> piece_first, piece_fin, piece_fout;
    std::vector<int64_t> piece_dst, piece_len, piece_src;
    size_t pieces() const { return piece_first.empty() ? (size_t)B : piece_dst.size(); }
};

// Fills p from B members of whole lengths member_len (each in [0, W_out]) and durations member_dur (may be null with STN_JOIN_WHOLE:
// prog_dur is then zero) at rate hz.  Empty string, or why the arguments are refused (p is then untouched).
std::string join_plan(const stn_join* j, int B, int64_t W_out, int hz, const int64_t* member_len, const float* member_dur, JoinPlan& p);

}  // namespace stn
