// pause_plan_check.cpp — stn_pause_plan (csrc/host/pause_plan.cpp) as a stand-alone program for the sanitizer build (make pause-asan:
// build_asan/pause_plan_check, -fsanitize=address,undefined).  It feeds the rule the cases of tests/test_pause_cpu.py and compares every
// result with a second, sample-by-sample implementation: each sample of the row is marked kept or dropped, and the cuts are read back
// from the marks.  Exit code 0 and "pause_plan_check OK" when all agree.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stn.h"

namespace {

int failures = 0;

struct Case { const char* name; int hz; int64_t K, n_short; std::vector<int64_t> active; float max_pause_ms; int want_cuts; };

// the rule, sample by sample: a sample of an inactive frame between two active ones is a pause sample; of every pause longer than Mp the
// first hl and the last hr samples stay
void brute(const Case& c, const std::vector<double>& lev, int64_t n, std::vector<int64_t>& cuts) {
    const int64_t F = (c.hz + 50) / 100, Mp = (int64_t)((double)c.max_pause_ms * c.hz / 1000.0 + 0.5);
    double mx = 0;
    for (double v : lev) mx = std::fmax(mx, v);
    cuts.clear();
    if (n == 0 || mx <= 1e-7) return;
    const double thr = mx * std::pow(10.0, -40.0 / 10.0);
    std::vector<char> act(lev.size());
    for (size_t k = 0; k < lev.size(); ++k) act[k] = lev[k] >= thr;
    std::vector<char> drop((size_t)n, 0);
    int64_t made = 0;
    for (int64_t k = 0; k < c.K;) {
        if (act[(size_t)k]) { ++k; continue; }
        int64_t e = k;
        while (e < c.K && !act[(size_t)e]) ++e;
        const bool inside = k > 0 && e < c.K;  // (a run that starts at frame 0 or reaches the last frame touches no active frame there)
        if (inside && (e - k) * F > Mp && made < 255) {
            for (int64_t s = k * F + (Mp - Mp / 2); s < e * F - Mp / 2; ++s) drop[(size_t)s] = 1;
            ++made;
        }
        k = e;
    }
    for (int64_t s = 0; s < n;) {
        if (!drop[(size_t)s]) { ++s; continue; }
        int64_t e = s;
        while (e < n && drop[(size_t)e]) ++e;
        cuts.push_back(s); cuts.push_back(e);
        s = e;
    }
}

void run(const Case& c) {
    const int64_t F = (c.hz + 50) / 100, n = c.K * F - c.n_short;
    std::vector<double> lev((size_t)c.K, 1e-8);
    for (int64_t k : c.active) lev[(size_t)k] = 0.04;
    std::vector<int64_t> want;
    brute(c, lev, n, want);
    // an exactly sized table: one pair more would be an overrun the sanitizer reports
    std::vector<int64_t> cuts(want.size());
    int64_t start = -1, end = -1;
    int32_t nc = -1;
    const int rc = stn_pause_plan(c.hz, n, lev.data(), c.K, 40.0f, 20.0f, c.max_pause_ms, &start, &end, cuts.empty() ? nullptr : cuts.data(),
                                  (int)(cuts.size() / 2), &nc);
    const bool ok = rc == STN_OK && nc == c.want_cuts && (int64_t)want.size() == 2 * (int64_t)nc && cuts == want && start >= 0 && end <= n && start <= end;
    std::printf("%-44s rc %d, %d cuts (designed %d), [%lld, %lld) of %lld: %s\n", c.name, rc, (int)nc, c.want_cuts, (long long)start, (long long)end,
                (long long)n, ok ? "ok" : "MISMATCH");
    if (!ok) ++failures;
    // null outputs and a table of zero pairs
    if (stn_pause_plan(c.hz, n, lev.data(), c.K, 40.0f, 20.0f, c.max_pause_ms, nullptr, nullptr, nullptr, 0, nullptr) != STN_OK) ++failures;
}

}  // namespace

int main() {
    std::vector<int64_t> many;
    for (int i = 0; i <= 300; ++i) many.push_back(4 * i);
    const Case cases[] = {
        {"P == Mp untouched, a longer one cut", 8000, 40, 3, {5, 6, 14, 30}, 70.0f, 1},
        {"P == Mp alone", 16000, 40, 3, {5, 6, 14}, 70.0f, 0},
        {"P == Mp + F", 48000, 40, 3, {5, 6, 15}, 70.0f, 1},
        {"odd Mp: hl = hr + 1", 11025, 50, 7, {2, 20, 21, 40}, 33.3f, 2},
        {"runs before f0 and behind f1 are no pauses", 16000, 100, 11, {30, 31, 32, 50, 51, 59}, 100.0f, 1},
        {"one active frame", 16000, 100, 11, {44}, 20.0f, 0},
        {"no speech", 16000, 100, 11, {}, 20.0f, 0},
        {"300 cuttable pauses: the first 255", 8000, 1206, 9, many, 20.0f, 255},
        {"a short last frame that closes a pause", 44100, 30, 440, {3, 29}, 50.0f, 1},
    };
    for (const Case& c : cases) run(c);
    // an empty row, and the refusals
    int64_t s = -1, e = -1;
    int32_t nc = -1;
    if (stn_pause_plan(8000, 0, nullptr, 0, 40.0f, 20.0f, 20.0f, &s, &e, nullptr, 0, &nc) != STN_OK || s != 0 || e != 0 || nc != 0) ++failures;
    const double lev[2] = {0.04, 0.04};
    if (stn_pause_plan(8000, 160, lev, 2, 40.0f, 20.0f, 19.0f, &s, &e, nullptr, 0, &nc) != STN_ERR_INVALID) ++failures;
    if (stn_pause_plan(8000, 160, lev, 2, 40.0f, 20.0f, 5001.0f, &s, &e, nullptr, 0, &nc) != STN_ERR_INVALID) ++failures;
    if (stn_pause_plan(8000, 161, lev, 2, 40.0f, 20.0f, 20.0f, &s, &e, nullptr, 0, &nc) != STN_ERR_INVALID) ++failures;
    if (stn_pause_plan(8000, 160, lev, 2, 40.0f, 20.0f, 20.0f, &s, &e, nullptr, 3, &nc) != STN_ERR_INVALID) ++failures;
    if (stn_pause_plan_error()[0] == 0) ++failures;
    if (failures) std::printf("pause_plan_check: %d FAILED\n", failures);
    else std::printf("pause_plan_check OK\n");
    return failures ? 1 : 0;
}
