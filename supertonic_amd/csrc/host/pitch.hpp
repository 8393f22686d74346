// pitch.hpp — the pitch shift's host arithmetic (include/stn.h "pitch"): the ratio a / b of a shift in semitones,
// the stretcher's geometry at a rate and its window.  Host only: no device, no handle.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace stn {

constexpr int PITCH_MAX_TERM = 640;  // a and b: what the resampler takes as P (RESAMPLE_MAX_P, kernels.hpp)

// why `semitones` is refused, or "": finite and in [-12, 12]
std::string pitch_check(float semitones);
// the fraction a / b, 1 <= a, b <= 640, closest to r = pow(2, semitones / 12) in log ratio (the smaller of q / r and r / q for q = a / b
// in double); of equals the smaller b, which is the reduced one.  false: pitch_check refuses the value
bool pitch_ratio(float semitones, int& a, int& b);

// WSOLA geometry at hz: H the smallest power of two with 128 H >= hz, N = 2 H, delta = 3 H / 4; over rows of W samples stretched by
// a / b: Ws = ceil(W a / b) and M = Ws / H + 2 frames
struct PitchPlan { int H = 0, delta = 0; int64_t M = 0, Ws = 0; };
std::string pitch_plan(int hz, int64_t W, int a, int b, PitchPlan& p);  // "" or why (hz outside [8000, 192000], W < 0, a or b outside [1, 640])
int pitch_hop(int hz);
// the periodic Hann of N = 2 H points, float32(0.5 (1 - cos(2 pi i / N))) in double
std::vector<float> pitch_window(int hz);

}  // namespace stn
