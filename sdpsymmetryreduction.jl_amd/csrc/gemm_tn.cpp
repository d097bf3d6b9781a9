// C = A' B on the host side: the split-K form of the MFMA product for skinny outputs and the exact-shape Gram product
// (callers: eigen.cpp, compress.cpp).
#include "host_internal.h"

namespace sdpsr {

// C = A' B for skinny outputs: the 128 x 128 output tiling alone would occupy a handful of
// CUs, so K is split over the batch dimension of the same MFMA kernel and the partial tiles are
// summed in fixed order.  Requires ldc == m (dense C) -- true for every caller.  `partials` names the ctx buffer of
// the partial tiles: a caller whose products run on the side stream beside the main stream's passes its own.
int gemm_tn_splitk(sdpsr_ctx* c, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* B,
                   int64_t ldb, double* C, int64_t ldc, const char* partials) {
    const int64_t tiles = (m / 128) * (n / 128);
    // K is split over Z workgroups per output tile: the largest divisor of the K-tile count that keeps
    // >= 128 of K per workgroup and the launch within ~one workgroup per CU (any divisor, not only
    // powers of two: ld = 4224 = 33 * 128 at N = 4104 has 264 = 8 * 33 K-tiles)
    int Z = 1;
    {
        const int64_t kt = k / 16;
        for (int64_t z = 1; z <= kt && tiles * z <= 256; ++z)
            if (kt % z == 0 && k / z >= 128) Z = (int)z;
    }
    if (Z == 1 || ldc != m) {
        launch_gemm_tn_f64(c->stream, m, n, k, A, lda, B, ldb, C, ldc, 1, 0, 0, 0);
        return SDPSR_OK;
    }
    double* P = (double*)ctx_buf(c, partials, (size_t)Z * m * n * 8);
    if (!P) return SDPSR_OUT_OF_MEMORY;
    const int64_t kz = k / Z;
    launch_gemm_tn_f64(c->stream, m, n, kz, A, lda, B, ldb, P, m, Z, kz, kz, m * n);
    launch_splitk_reduce(c->stream, m * n, Z, m * n, P, C);
    return SDPSR_OK;
}

// The route of gram_tn: true when both operands fit the LDS stage of the skinny Gram kernel (32 rows of each, pitch = the
// columns rounded up to 16, + 1; (128, 112) is the last shape that fits 64 KiB), false for the padded split-K MFMA product.
bool gram_tn_is_skinny(int64_t ma, int64_t nb) {
    const int64_t pa = (ma + 15) / 16 * 16 + 1, pb = (nb + 15) / 16 * 16 + 1;
    return ma >= 1 && nb >= 1 && ma <= 128 && nb <= 128 && 32 * (pa + pb) * 8 <= 64 * 1024;
}

// C = A' B of the exact shape ma x nb (A: k x ma, B: k x nb) into the mp x np padded result, zero
// outside ma x nb: the skinny Gram kernel when both operands fit its LDS stage (gram_tn_is_skinny), the padded
// split-K MFMA product otherwise.  The two routes keep "zero outside ma x nb" differently.  The skinny kernel
// reads the columns < ma of A and < nb of B only and WRITES the zeros.  The split-K product multiplies all
// mp columns of A by all np columns of B (mp, np multiples of 128, k a multiple of 128): its padding is the
// product of the operands' padding columns, so there the caller must hold A zero in columns ma..mp and B zero in
// columns nb..np (compress.cpp clears W and T before it fills them).
int gram_tn(sdpsr_ctx* c, int64_t ma, int64_t nb, int64_t k, const double* A, int64_t lda, const double* B, int64_t ldb,
            double* C, int64_t mp, int64_t np, double* host_C, bool* host_filled) {
    if (host_filled) *host_filled = false;
    if (gram_tn_is_skinny(ma, nb)) {
        double* P = (double*)ctx_buf(c, "gram_partials", gram_small_partial_doubles(k, (int)ma, (int)nb) * 8);
        if (!P) return SDPSR_OUT_OF_MEMORY;
        launch_gram_small(c->stream, k, (int)ma, (int)nb, A, lda, B, ldb, P, C, mp, (int)mp, (int)np, host_C);
        if (host_filled) *host_filled = host_C != nullptr;
        return SDPSR_OK;
    }
    return gemm_tn_splitk(c, mp, np, k, A, lda, B, ldb, C, mp);
}

}  // namespace sdpsr
