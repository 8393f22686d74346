// engine_internal.hpp — helpers shared by the engine's translation units (engine.cpp: lifecycle, weights, blocks and the four stages;
// engine_batch.cpp: the resident-batch pipeline and its graph cache; engine_ops.cpp: the single-kernel and timing entry points of the tests
// and tools).
#pragma once
#include "engine.hpp"

#include <algorithm>
#include <cstdio>

namespace stn {
namespace detail {
// host array -> arena (asynchronous copy on `s`)
template <typename T>
inline T* up(Arena& ar, hipStream_t s, const T* h, size_t n) {
    T* d = static_cast<T*>(ar.alloc(n * sizeof(T)));
    STN_HIP(hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s));
    return d;
}
}  // namespace detail

// a number as the refusals print it
inline std::string num(double v) {
    char b[48];
    std::snprintf(b, sizeof(b), "%g", v);
    return b;
}

// why a setting of `unit` is refused, or "": the first field outside its range, "<unit>: <name> <v> must be in [<lo>, <hi>]"
struct Lim { const char* name; float v, lo, hi; };
template <size_t N>
inline std::string range_check(const char* unit, const Lim (&lim)[N]) {
    for (const Lim& l : lim)  // (a NaN fails both comparisons)
        if (!(l.v >= l.lo && l.v <= l.hi)) return std::string(unit) + ": " + l.name + " " + num(l.v) + " must be in [" + num(l.lo) + ", " + num(l.hi) + "]";
    return "";
}

// The rows of an op-level entry on the device, from the engine's arena: [guard][x][guard] and [guard][y][guard] (in place: one block),
// the blocks filled with the quiet NaN 0x7FC00000 when probing, both 4 bytes off a 16-byte boundary when misaligned (the arena's blocks
// are 256-byte aligned).  x is uploaded; the caller's launches read dx and write dy.
struct GuardedRows {
    static constexpr size_t G = 64;
    Engine& e;
    size_t nx, off;
    float *bx, *by, *dx, *dy;
    GuardedRows(Engine& eng, size_t n, const float* x, bool probing, bool misalign, bool in_place) : e(eng), nx(n), off(misalign ? 1 : 0) {
        bx = static_cast<float*>(e.arena().alloc((nx + 2 * G + off) * 4));
        by = in_place ? bx : static_cast<float*>(e.arena().alloc((nx + 2 * G + off) * 4));
        dx = bx + G + off;
        dy = by + G + off;
        if (probing)
            for (float* b : {bx, by}) STN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b), 0x7FC00000, nx + 2 * G + off, e.stream()));
        STN_HIP(hipMemcpyAsync(dx, x, nx * 4, hipMemcpyHostToDevice, e.stream()));
    }
    void download(float* y) const { STN_HIP(hipMemcpyAsync(y, dy, nx * 4, hipMemcpyDeviceToHost, e.stream())); }
    // every guard word still holds the poison (waits for the stream)
    bool guards_ok() const {
        std::vector<uint32_t> g(4 * G + 2 * off);
        uint32_t* p = g.data();
        for (float* b : {bx, by}) {
            STN_HIP(hipMemcpyAsync(p, b, (G + off) * 4, hipMemcpyDeviceToHost, e.stream()));
            STN_HIP(hipMemcpyAsync(p + G + off, b + G + off + nx, G * 4, hipMemcpyDeviceToHost, e.stream()));
            p += 2 * G + off;
        }
        e.sync();
        return std::all_of(g.begin(), g.end(), [](uint32_t v) { return v == 0x7FC00000u; });
    }
};
}  // namespace stn
