// Host arithmetic of the on-device canonical pass of a sparse-constraints handle (sparse_handle.cpp, kernels_csr_canon.hip):
// the verdict words the kernels report, which message they mean (the precedence of canonicalize_csr's own checks), the
// radix bits of the two sorts and the chunk count of the compaction.  Plain C++: tested as a program of its own.
#pragma once
#include <cstdint>
#include <string>

namespace sdpsr {

// One 64-bit word per verdict, in device memory while the pass runs and read back through the ctx's pinned words.
// bad_row / bad_col / bad_val: the lowest offending index (integer atomicMin), CANON_NO_INDEX = none; the others: != 0 = raised.
struct CanonVerdict {
    unsigned long long bad_row;        // lowest row i with rowptr[i + 1] < rowptr[i]
    unsigned long long bad_col;        // lowest entry p with a column outside [0, len)
    unsigned long long bad_val;        // lowest entry p with a non-finite value
    unsigned long long rowptr0_bad;    // rowptr[0] != index_base
    unsigned long long nnz_mismatch;   // rowptr[m] - index_base != nnz
    unsigned long long unsorted;       // some row is not strictly increasing: the sort runs
    unsigned long long dup_nonfinite;  // a run of duplicates sums to a non-finite value
    unsigned long long asymmetric;     // some row is not a symmetric matrix bit for bit
    unsigned long long total;          // canonical entries
};
constexpr unsigned long long CANON_NO_INDEX = ~0ull;

// The message of the first check canonicalize_csr would have failed, "" if it would have passed its validation loop:
// rowptr[0], then the lowest non-monotone row, then (new with an explicit nnz) the length, then the lowest offending entry
// of either kind -- the host loop tests the column of an entry before its value, so the column wins at equal p.
inline std::string canon_validation_message(const CanonVerdict& v) {
    if (v.rowptr0_bad) return "rowptr[0] != index_base";
    if (v.bad_row != CANON_NO_INDEX) return "rowptr is not monotone at row " + std::to_string(v.bad_row);
    if (v.nnz_mismatch) return "rowptr[m] - index_base != nnz";
    if (v.bad_col != CANON_NO_INDEX && v.bad_col <= v.bad_val) return "column index out of [0, n^2) at entry " + std::to_string(v.bad_col);
    if (v.bad_val != CANON_NO_INDEX) return "non-finite value at entry " + std::to_string(v.bad_val);
    return "";
}

// bits of a stable LSD radix sort whose keys are 0 .. count - 1 (at least one pass: the sort's output buffers are written)
inline int canon_sort_bits(uint64_t count) {
    int l = 1;
    while (l < 64 && (uint64_t(1) << l) < count) ++l;
    return l;
}

// the compaction scans fixed chunks of positions: count per chunk, int64 scan over the chunks, fill
constexpr int64_t CANON_CHUNK = 2048;
inline int64_t canon_chunks(int64_t n) { return n <= 0 ? 0 : (n + CANON_CHUNK - 1) / CANON_CHUNK; }

// perfect-square root of len, or 0: rows can only be symmetric matrices when len = n^2
inline int64_t canon_square_root(int64_t len) {
    if (len < 1) return 0;
    int64_t n = 0;
    for (int64_t bit = int64_t(1) << 31; bit > 0; bit >>= 1)
        if ((n + bit) <= len / (n + bit)) n += bit;
    return n * n == len ? n : 0;
}

}  // namespace sdpsr
