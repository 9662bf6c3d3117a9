// A batch of ragged arrays, as every registration entry point takes it: int64 offsets of n + 1 entries, member c holds the
// rows [off[c], off[c + 1]).  Here is the one statement of how such offsets are checked and measured, and of how a scratch
// block is cut into 256-byte-aligned pieces.  Plain C++ without HIP, so that it can also be compiled into a stand-alone
// program and run under host sanitizers.  The messages and the device-side half are in common.h.
#pragma once
#include <stdint.h>
#include <stddef.h>

struct RaggedShape {
    int64_t total;               // off[n]: the rows the arrays hold
    int64_t largest, smallest;   // member lengths; both 0 when n is 0
};

enum { RAGGED_OK = 0, RAGGED_E_START = 1, RAGGED_E_DECREASE = 2 };

// any_start = 0: the offsets start at row 0 exactly; 1: at any row >= 0.  The limits of a caller (no empty member, an
// int32 index range, ...) are the caller's own checks on what is measured here.
static inline int ragged_measure(const int64_t *off, int n, int any_start, RaggedShape *s) {
    if (any_start ? off[0] < 0 : off[0] != 0) return RAGGED_E_START;
    s->total = off[n];
    s->largest = 0;
    s->smallest = n > 0 ? INT64_MAX : 0;
    for (int c = 0; c < n; ++c) {
        if (off[c + 1] < off[c]) return RAGGED_E_DECREASE;
        const int64_t len = off[c + 1] - off[c];
        if (len > s->largest) s->largest = len;
        if (len < s->smallest) s->smallest = len;
    }
    return RAGGED_OK;
}

// Cuts one block into pieces that each start on a multiple of 256 bytes.  A layout is a function of the carver: called
// with a null base it only sizes (every piece is null, `at` ends as the bytes needed), called again with the block it
// places the same pieces, so the size and the placement cannot drift apart.
struct Carver {
    char *base;
    size_t at = 0;
    explicit Carver(void *b = nullptr) : base((char *)b) {}
    template <typename T> T *take(size_t count, size_t slack_bytes = 0) {
        T *r = base ? (T *)(base + at) : nullptr;
        at += (count * sizeof(T) + slack_bytes + 255) / 256 * 256;
        return r;
    }
};
