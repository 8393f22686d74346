// formant.hpp — the formant correction's host arithmetic (include/stn.h "formant"): the geometry at a rate, the lag
// window, and the conditioning and Levinson-Durbin recursion in double.  Host only: no device, no handle.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace stn {

constexpr int FORMANT_MAX_ORDER = 48;

// hop H (the pitch stage's), order p = min(48, max(10, 2 ceil(hz / 2000) + 2)), frames m = 0 .. ceil(W / H): ceil(W / H) + 1 of them
struct FormantPlan { int H = 0, p = 0; int64_t frames = 0; };
std::string formant_plan(int hz, int64_t W, FormantPlan& f);  // "" or why (hz outside [8000, 192000], W outside [0, 2^40])
// the Gaussian lag window in double, p + 1 values: 1 at lag 0, exp(-0.5 (2 pi 60 k / hz)^2) at lag k
std::vector<double> formant_lag_window(int hz, int p);
// r[0 .. p] -> a[0 .. p] (a[0] = 1) and the final error: r'[0] = 1.0001 r[0] + 1e-9, r'[k] = r[k] lagw[k], then Levinson-Durbin.
// refl (or null): the p reflection coefficients
void formant_lpc(const double* r, const double* lagw, int p, double* a, double* err, double* refl);

}  // namespace stn
