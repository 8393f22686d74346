// pause_plan.hpp — the pause limit's rule on the host (include/stn.h, "pause limit"): from a row's frame levels
// to its edges and the cuts that shorten every pause inside it to max_pause.  Host arithmetic only: stn_pause_plan, the engine's
// setter and table sizing, and the join plan share it.  The kernel (pause_rows_kernel, kernels_edges.hip) computes the same integers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace stn {

constexpr int PAUSE_MAX_CUTS = 255;  // cuts made per row: the first 255 in time order

struct PauseCut { int64_t lo, hi; };  // the dropped samples [lo, hi)

struct PausePlan {
    int64_t start = 0, end = 0;   // section 14's edges
    int64_t len = 0;              // end - start minus what the cuts drop
    std::vector<PauseCut> cuts;   // ascending, at most PAUSE_MAX_CUTS
};

std::string pause_check(float max_pause_ms);  // empty, or why the value is refused ([20, 5000])
// (int64)(max_pause_ms * hz / 1000 + 0.5), in double
int64_t pause_samples(int hz, float max_pause_ms);
// table words per row: one more than the cuts a row of W samples can hold (a cut needs a pause longer than Mp and an active frame
// behind it), 256 at the most
int pause_stride(int64_t W, int hz, int64_t Mp);
// n samples in frames of F = (hz + 50) / 100 with levels level[K], K = ceil(n / F); keep and Mp in samples
PausePlan pause_plan(int hz, int64_t n, const double* level, int64_t K, double top_db, int64_t keep, int64_t Mp);

// the row's segments as the store takes them: [start, lo_0), [hi_0, lo_1), ..., [hi_m-1, end) laid end to end from column 0; an edge made
// by a cut, and start > 0 and end < n, is faded over min(fd, len) samples
struct PausePiece { int64_t dst, len, src; int32_t fin, fout; };
std::vector<PausePiece> pause_pieces(int64_t start, int64_t end, int64_t n, const int64_t* cuts, int m, int64_t fd);

}  // namespace stn
