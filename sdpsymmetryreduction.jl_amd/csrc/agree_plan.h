// The decisions of the restarts' agreement (agree.cpp) as plain host arithmetic: plain C++17, no HIP, tested alone
// (tests/test_agree_plan_cpu.py).  Every rank holds R restarts of one reduction; a restart is a SLOT, numbered rank * R + i
// over all ranks.  The ranks exchange one fixed-size record each and every rank takes the same decision from the same table.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdpsr {

constexpr int AGREE_MAX_RESTARTS = 64;  // the batch entries' limit

// the multiplier of slot k in the meet's keys, key[e] = sum_k label_k[e] * m(k) mod 2^64: the eight odd constants of
// parallel.py (_ODD), times the odd numbers 1, 3, 5, ... from the ninth slot on.  Odd, so label * m(k) is injective in the label.
constexpr uint64_t AGREE_ODD[8] = {0x9E3779B97F4A7C15ull, 0xBF58476D1CE4E5B9ull, 0x94D049BB133111EBull, 0xD6E8FEB86659FD93ull,
                                   0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull, 0x85EBCA77C2B2AE63ull};
inline uint64_t agree_multiplier(uint64_t k) { return AGREE_ODD[k % 8] * (2 * (k / 8) + 1); }

// first slot of a rank: its restarts take the slots first_slot .. first_slot + R - 1
inline int64_t agree_first_slot(int32_t rank, int32_t R) { return (int64_t)rank * R; }

// what a rank contributes to the table: 64-bit words only, the same size on every rank whatever its R (a rank whose R differs
// must still be able to take part in the gather that finds that out)
struct AgreeRecord {
    int64_t len = 0;
    int64_t R = 0;
    int64_t width = 0;  // bits of a label (8 / 16 / 32)
    int64_t reserved = 0;
    uint64_t valid[AGREE_MAX_RESTARTS] = {};  // != 0: the restart's labels are a partition (status OK / the randomized failures of blockDiagonalize)
    uint64_t word0[AGREE_MAX_RESTARTS] = {};  // sdpsr_partition_checksum of the restart's labels
    uint64_t word1[AGREE_MAX_RESTARTS] = {};
};
static_assert(sizeof(AgreeRecord) == 32 + 3 * 8 * AGREE_MAX_RESTARTS, "AgreeRecord is gathered as bytes: no padding");

enum AgreePlan {
    AGREE_MISMATCH = 0,    // some rank's len, R or width differs (or an R outside 1 .. 64): SDPSR_BAD_ARGUMENT on every rank
    AGREE_NONE_VALID = 1,  // no valid restart anywhere: SDPSR_BAD_STATE
    AGREE_AGREED = 2,      // every restart of every rank valid and all checksums equal: nothing to do
    AGREE_MEET = 3         // anything else: the meet of the valid restarts goes into every array
};

// records: `world` of them, in rank order (the gathered table; world = 1: the local record)
inline AgreePlan agree_plan(int32_t world, const AgreeRecord* rec) {
    if (world < 1 || rec[0].R < 1 || rec[0].R > AGREE_MAX_RESTARTS) return AGREE_MISMATCH;
    for (int32_t r = 1; r < world; ++r)
        if (rec[r].len != rec[0].len || rec[r].R != rec[0].R || rec[r].width != rec[0].width) return AGREE_MISMATCH;
    const int R = (int)rec[0].R;
    int64_t nvalid = 0;
    bool equal = true;
    uint64_t w0 = 0, w1 = 0;  // the first valid restart's words (an invalid restart's words mean nothing)
    for (int32_t r = 0; r < world; ++r)
        for (int i = 0; i < R; ++i) {
            if (!rec[r].valid[i]) continue;
            if (nvalid++ == 0) {
                w0 = rec[r].word0[i];
                w1 = rec[r].word1[i];
            }
            if (rec[r].word0[i] != w0 || rec[r].word1[i] != w1) equal = false;
        }
    if (nvalid == 0) return AGREE_NONE_VALID;
    if (nvalid == (int64_t)world * R && equal) return AGREE_AGREED;
    return AGREE_MEET;  // (an invalid restart beside agreeing ones too: it has to receive the partition)
}

// blockDiagonalize's side: the lowest rank whose status is 0 (SDPSR_OK) wins; -1: every rank failed
inline int32_t agree_winner(int32_t world, const int32_t* status) {
    for (int32_t r = 0; r < world; ++r)
        if (status[r] == 0) return r;
    return -1;
}

}  // namespace sdpsr
