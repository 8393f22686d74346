// join_plan.cpp — see join_plan.hpp.
#include "join_plan.hpp"

#include <algorithm>

namespace stn {

std::string join_plan(const stn_join* j, int B, int64_t W_out, int hz, const int64_t* member_len, const float* member_dur, JoinPlan& out) {
    if (!j) return "join: null description";
    if (j->n_prog < 1) return "join: n_prog = " + std::to_string(j->n_prog) + " (at least one programme)";
    if (!j->rows || !j->gap_samples) return "join: rows and gap_samples must be given";
    if (j->mode != STN_JOIN_WHOLE && j->mode != STN_JOIN_TRIM) return "join: unknown mode " + std::to_string(j->mode);
    if (j->gain_scope != STN_JOIN_GAIN_ROW && j->gain_scope != STN_JOIN_GAIN_PROG) return "join: unknown gain scope " + std::to_string(j->gain_scope);
    if (B < 1 || W_out < 0 || !member_len) return "join: no members";
    if (member_dur && !j->gap_seconds) return "join: gap_seconds must be given";
    if (j->mode == STN_JOIN_TRIM && (!member_dur || hz <= 0)) return "join: trimming needs the members' durations and the rate";
    int64_t sum = 0;
    for (int g = 0; g < j->n_prog; ++g) {
        if (j->rows[g] < 1) return "join: programme " + std::to_string(g) + " has " + std::to_string(j->rows[g]) + " members (at least one)";
        if (j->gap_samples[g] < 0) return "join: programme " + std::to_string(g) + " has a negative gap (" + std::to_string(j->gap_samples[g]) + " samples)";
        sum += j->rows[g];
        if (sum > B) break;
    }
    if (sum != B) return "join: the programmes' members sum to " + std::string(sum > B ? "more than " : "") + std::to_string(sum > B ? B : sum) +
                         " but the batch has " + std::to_string(B) + " rows";
    for (int i = 0; i < B; ++i)
        if (member_len[i] < 0 || member_len[i] > W_out)
            return "join: member " + std::to_string(i) + " has length " + std::to_string(member_len[i]) + " outside [0, " + std::to_string(W_out) + "]";
    JoinPlan p;
    p.G = j->n_prog; p.B = B;
    p.first.resize((size_t)p.G);
    p.seg_len.resize((size_t)B); p.seg_dst.resize((size_t)B);
    p.prog_len.resize((size_t)p.G); p.prog_dur.assign((size_t)p.G, 0.f);
    int i = 0;
    for (int g = 0; g < p.G; ++g) {
        p.first[(size_t)g] = i;
        int64_t at = 0;
        float d = 0.f;
        for (int m = 0; m < j->rows[g]; ++m, ++i) {
            int64_t len = member_len[i];
            if (j->mode == STN_JOIN_TRIM) {  // rust/src/helper.rs:700-702: (sample_rate * duration) as usize, the product in fp32
                const float f = member_dur[i] * (float)hz;
                if (!(f > 0.f)) len = 0;
                else if (f < (float)len) len = (int64_t)f;
            }
            if (m > 0) at += j->gap_samples[g];
            p.seg_dst[(size_t)i] = at;
            p.seg_len[(size_t)i] = len;
            at += len;
            if (member_dur) {  // cpp/helper.cpp:708,714: fp32, in member order
                if (m == 0) d = member_dur[i];
                else d += member_dur[i] + j->gap_seconds[g];
            }
        }
        p.prog_len[(size_t)g] = at;
        p.prog_dur[(size_t)g] = d;
        p.W_join = std::max(p.W_join, at);
    }
    out = std::move(p);
    return "";
}

}  // namespace stn

static thread_local std::string g_join_err;

extern "C" {

const char* stn_join_plan_error(void) { return g_join_err.c_str(); }

int stn_join_plan(const stn_join* j, int B, int64_t W_out, int hz, const int64_t* member_len, const float* member_dur, int64_t* W_join,
                  int64_t* prog_len, float* prog_dur, int64_t* seg_len, int64_t* seg_dst) {
    try {
        stn::JoinPlan p;
        g_join_err = stn::join_plan(j, B, W_out, hz, member_len, member_dur, p);
        if (!g_join_err.empty()) return STN_ERR_INVALID;
        if (W_join) *W_join = p.W_join;
        if (prog_len) std::copy(p.prog_len.begin(), p.prog_len.end(), prog_len);
        if (prog_dur) std::copy(p.prog_dur.begin(), p.prog_dur.end(), prog_dur);
        if (seg_len) std::copy(p.seg_len.begin(), p.seg_len.end(), seg_len);
        if (seg_dst) std::copy(p.seg_dst.begin(), p.seg_dst.end(), seg_dst);
        return STN_OK;
    } catch (const std::exception& e) {
        g_join_err = e.what();
        return STN_ERR_INVALID;
    }
}

}  // extern "C"
