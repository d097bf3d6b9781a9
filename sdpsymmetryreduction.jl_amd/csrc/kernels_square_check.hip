// "Is X_t^2 constant on the classes?" without forming X_t^2 (deviation 15).
// A round that is expected not to refine wants one bit per round: does the square of the random element X_t (X_t[i,j] = the int8 value of
// class L[i,j] in channel t, 0 on label 0) take, on every entry, the value it takes at the representative of the entry's class (0 on label 0)?
// With c_t[k] = (X_t^2)[first_idx[k-1]] and C_t[i,j] = c_t[L[i,j]] that is the identity X_t^2 = C_t between two SYMMETRIC integer matrices,
// and D = X_t^2 - C_t = 0 is tested with a random vector v in {0 .. 2^16 - 1}^n:  v'Dv = |X_t v|^2 - v'(C_t v) is a polynomial of degree 2
// in v that is not the zero polynomial when D != 0, so it vanishes with probability <= 2 / 2^16 (Schwartz-Zippel); "violated" is never
// false.  Everything is exact integer arithmetic, O(n^2) operations on the packed labels, no int8 matrix and no int32 product:
//   square_check_ref_kernel      c[g][t][k]: one workgroup per class, the 2 n label reads of row i and column j of the representative for both rounds
//   square_check_pass_kernel     ONE pass over the packed labels, the tile-pair walk of gather_i8_sym_packed_kernel: writes the full label
//                                matrix (WRITE_L) and, per 64 x 64 tile, the tile's share of X_t v and C_t v (rows, and columns for the
//                                mirrored tile) into part[column block][row]: every slot has one owner, no atomics, no fills
//   square_check_rows_kernel     y = sum_b part_x[b], w = sum_b part_c[b] and, per 64 rows, the 128-bit sum of y_i^2 - v_i w_i
//   square_check_verdict_kernel  adds those sums; a non-zero one stores 1 into its round's verdict word (never 0: the host cleared it)
// G <= 2 rounds (keys), T = 2 or 4 channels each, d <= 255 classes, n <= 2^15 (|c| <= 2^14 n fits int32; the x sums of a tile are below
// 2^7 2^16 2^6, the c sums below 2^29 2^16 2^6).  The x products stay on the 24-bit multiply-add (full rate); c v is one 32 x 32 -> 64 one.
#include "host_internal.h"
#include "sdpsr_hash.h"

namespace sdpsr {

namespace {

constexpr int CHECK_TILE = 64;

// (i, j), i >= j, of packed index e < n (n + 1) / 2 (column j starts at j n - j (j - 1) / 2)
__device__ __forceinline__ void check_packed_ij(int n, int64_t e, int& i, int& j) {
    const float t = (float)(2 * n + 1);
    int jj = (int)((t - sqrtf(fmaxf(t * t - 8.0f * (float)e, 0.0f))) * 0.5f);
    jj = jj < 0 ? 0 : (jj > n - 1 ? n - 1 : jj);
    while ((int64_t)jj * n - (int64_t)jj * (jj - 1) / 2 > e) --jj;
    while (jj + 1 < n && (int64_t)(jj + 1) * n - (int64_t)(jj + 1) * jj / 2 <= e) ++jj;
    j = jj;
    i = jj + (int)(e - ((int64_t)jj * n - (int64_t)jj * (jj - 1) / 2));
}
// label of entry (a, b) of the symmetric matrix, from the packed lower triangle
template <typename LT>
__device__ __forceinline__ uint32_t check_label(const LT* __restrict__ Lp, int n, int a, int b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    return (uint32_t)Lp[(int64_t)lo * n - (int64_t)lo * (lo - 1) / 2 + (hi - lo)];
}

// One workgroup of REF_THREADS per class serves both rounds from the same label reads (the labels of row i above the diagonal are n
// bytes apart: every lane its own cache line), REF_UNROLL entries of the row and of the column in flight per thread.  int32 sums:
// any order gives the same bits.
constexpr int REF_THREADS = 1024, REF_UNROLL = 4;
template <int T, typename LT>
__global__ void __launch_bounds__(REF_THREADS)
square_check_ref_kernel(int n, int d, int G, const LT* __restrict__ Lp, const uint32_t* __restrict__ first_idx, uint64_t key0, uint64_t key1,
                        int32_t* __restrict__ c) {
    __shared__ uint32_t xt[2][SQUARE_CHECK_MAX_CLASSES + 1];
    __shared__ int32_t red[REF_THREADS / 64][2 * T];
    const int k = blockIdx.x;
    for (int l = threadIdx.x; l < 2 * (SQUARE_CHECK_MAX_CLASSES + 1); l += blockDim.x) {
        const int g = l / (SQUARE_CHECK_MAX_CLASSES + 1), cl = l % (SQUARE_CHECK_MAX_CLASSES + 1);
        xt[g][cl] = (cl && cl <= d && g < G) ? (uint32_t)sdpsr_class_bits(g ? key1 : key0, (uint32_t)cl) : 0u;
    }
    __syncthreads();
    int32_t acc[2 * T];
#pragma unroll
    for (int a = 0; a < 2 * T; ++a) acc[a] = 0;
    const int64_t e = (int64_t)first_idx[k];
    if (e < (int64_t)n * (n + 1) / 2) {  // (a representative outside the triangle: the class constants stay 0)
        int i, j;
        check_packed_ij(n, e, i, j);
        for (int m0 = threadIdx.x; m0 < n; m0 += REF_UNROLL * (int)blockDim.x) {
            uint32_t la[REF_UNROLL], lb[REF_UNROLL];
#pragma unroll
            for (int u = 0; u < REF_UNROLL; ++u) {
                const int m = m0 + u * (int)blockDim.x;
                la[u] = m < n ? check_label(Lp, n, i, m) : 0u;  // (label 0: the channel bytes are 0, nothing is added)
                lb[u] = m < n ? check_label(Lp, n, m, j) : 0u;
            }
#pragma unroll
            for (int u = 0; u < REF_UNROLL; ++u) {
                const uint32_t a = la[u] <= (uint32_t)d ? la[u] : 0u, b = lb[u] <= (uint32_t)d ? lb[u] : 0u;
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const uint32_t xa = xt[g][a], xb = xt[g][b];
#pragma unroll
                    for (int t = 0; t < T; ++t) acc[g * T + t] += __mul24(sdpsr_class_i8(xa, t), sdpsr_class_i8(xb, t));
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 2 * T; ++a) {
        int v = acc[a];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][a] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < G * T) {  // (g, t) = threadIdx.x / T, threadIdx.x % T: row g T + t of c, as before
        int32_t v = 0;
        for (int w = 0; w < (int)blockDim.x / 64; ++w) v += red[w][threadIdx.x];
        c[(int64_t)threadIdx.x * d + k] = v;
    }
}

// what the pass looks up per (round, label): the channel bytes of the class and its T class constants
template <int T>
struct CheckClass {
    uint32_t xbits;
    int32_t c[T];
};

// One orientation of a staged tile: thread (r, p) adds the 16 entries 16 p .. 16 p + 15 of line r (ROWS: row r of the tile, weights vw = v of
// the tile's columns; else column r, weights v of its rows), the four p of a line are neighbouring lanes.  Lane p = 0 stores the line's sums.
template <int G, int T, bool ROWS>
__device__ __forceinline__ void check_tile_sums(const uint32_t (*tile)[CHECK_TILE + 1], const CheckClass<T> (*cls)[SQUARE_CHECK_MAX_CLASSES + 1],
                                                const uint32_t (*vw)[CHECK_TILE], int d, int32_t* __restrict__ part_x, int64_t* __restrict__ part_c,
                                                int64_t slot, int64_t gt_stride) {
    const int r = threadIdx.x >> 2, p = threadIdx.x & 3;
    int32_t sx[G * T];
    int64_t sc[G * T];
#pragma unroll
    for (int a = 0; a < G * T; ++a) sx[a] = 0, sc[a] = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int k = 16 * p + q;
        uint32_t l = ROWS ? tile[k][r] : tile[r][k];
        l = l <= (uint32_t)d ? l : 0u;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int v = (int)vw[g][k];
            const CheckClass<T> rec = cls[g][l];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                sx[g * T + t] += __mul24(sdpsr_class_i8(rec.xbits, t), v);
                sc[g * T + t] += (int64_t)rec.c[t] * (int64_t)v;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < G * T; ++a) {
        sx[a] += __shfl_xor(sx[a], 1);
        sx[a] += __shfl_xor(sx[a], 2);
        sc[a] += __shfl_xor((long long)sc[a], 1);
        sc[a] += __shfl_xor((long long)sc[a], 2);
    }
    if (p == 0) {
#pragma unroll
        for (int a = 0; a < G * T; ++a) {
            part_x[a * gt_stride + slot + r] = sx[a];
            part_c[a * gt_stride + slot + r] = sc[a];
        }
    }
}

// grid (nb, nb), nb = ceil(n / 64); tiles bi >= bj.  part_x / part_c: [G T][nb][nb 64].
template <int G, int T, bool WRITE_L, typename LT>
__global__ void __launch_bounds__(256)
square_check_pass_kernel(int n, int d, const LT* __restrict__ Lp, uint64_t key0, uint64_t key1, const int32_t* __restrict__ c,
                         uint32_t* __restrict__ Lfull, int32_t* __restrict__ part_x, int64_t* __restrict__ part_c) {
    __shared__ CheckClass<T> cls[G][SQUARE_CHECK_MAX_CLASSES + 1];
    __shared__ uint32_t vrow[G][CHECK_TILE], vcol[G][CHECK_TILE];  // v of the tile's rows i0 .. and of its columns j0 ..
    __shared__ uint32_t tile[CHECK_TILE][CHECK_TILE + 1];           // [column][row]: label of entry (i0 + row, j0 + column), 0 past n
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bi < bj) return;
    const int nb = gridDim.x;
    const int i0 = bi * CHECK_TILE, j0 = bj * CHECK_TILE;
    const uint64_t keys[2] = {key0, key1};
    {
        const int l = threadIdx.x;  // 256 threads, 256 slots
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const bool live = l >= 1 && l <= d;
            CheckClass<T> rec;
            rec.xbits = live ? (uint32_t)sdpsr_class_bits(keys[g], (uint32_t)l) : 0u;
#pragma unroll
            for (int t = 0; t < T; ++t) rec.c[t] = live ? c[(int64_t)(g * T + t) * d + (l - 1)] : 0;
            cls[g][l] = rec;
        }
        if (threadIdx.x < 2 * CHECK_TILE) {
            const int which = threadIdx.x >> 6, o = threadIdx.x & 63, idx = (which ? j0 : i0) + o;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const uint32_t v = idx < n ? sdpsr_check_vector(sdpsr_check_vector_key(keys[g]), (uint32_t)idx) : 0u;
                if (which) vcol[g][o] = v;
                else vrow[g][o] = v;
            }
        }
    }
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int i = i0 + tx, j = j0 + ty + 4 * q;
        uint32_t lab = 0u;
        if (i < n && j < n) {
            lab = check_label(Lp, n, i, j);  // (diagonal tiles: the upper half by symmetry)
            if (WRITE_L) Lfull[(int64_t)i + (int64_t)j * n] = lab;
        }
        tile[ty + 4 * q][tx] = lab;
    }
    __syncthreads();
    if (WRITE_L && bi != bj) {  // the mirrored tile: row j0 + tx, column i0 + cc  (= entry (i0 + cc, j0 + tx))
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int cc = ty + 4 * q, rr = j0 + tx, col = i0 + cc;
            if (rr < n && col < n) Lfull[(int64_t)rr + (int64_t)col * n] = tile[tx][cc];
        }
    }
    const int64_t npad = (int64_t)nb * CHECK_TILE, gt_stride = (int64_t)nb * npad;
    // rows i0 .. of the tile against the columns of block bj; off the diagonal also columns j0 .. (rows of the mirrored tile) against block bi
    check_tile_sums<G, T, true>(tile, cls, vcol, d, part_x, part_c, (int64_t)bj * npad + i0, gt_stride);
    if (bi != bj) check_tile_sums<G, T, false>(tile, cls, vrow, d, part_x, part_c, (int64_t)bi * npad + j0, gt_stride);
}

// 128-bit sum over the lanes of a wave (mod 2^128: any order gives the same bits); lane 0 holds it
__device__ __forceinline__ unsigned __int128 check_wave_sum128(unsigned __int128 e) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t lo = (uint64_t)__shfl_down((unsigned long long)(uint64_t)e, o), hi = (uint64_t)__shfl_down((unsigned long long)(uint64_t)(e >> 64), o);
        e += ((unsigned __int128)hi << 64) | (unsigned __int128)lo;
    }
    return e;
}

// grid (nb, G T), 256 threads = 64 rows x 4 slices of the column blocks.  esum: [G T][nb] 128-bit sums as (low, high) words.
__global__ void __launch_bounds__(256)
square_check_rows_kernel(int n, int nb, int T, uint64_t key0, uint64_t key1, const int32_t* __restrict__ part_x, const int64_t* __restrict__ part_c,
                         int64_t* __restrict__ y, int64_t* __restrict__ w, uint64_t* __restrict__ esum) {
    __shared__ int64_t sy[4][CHECK_TILE], sw[4][CHECK_TILE];
    const int r = threadIdx.x & 63, sl = threadIdx.x >> 6, gt = blockIdx.y;
    const int64_t npad = (int64_t)nb * CHECK_TILE, i = (int64_t)blockIdx.x * CHECK_TILE + r;
    int64_t ys = 0, ws = 0;
    for (int b = sl; b < nb; b += 4) {
        ys += (int64_t)part_x[((int64_t)gt * nb + b) * npad + i];
        ws += part_c[((int64_t)gt * nb + b) * npad + i];
    }
    sy[sl][r] = ys, sw[sl][r] = ws;
    __syncthreads();
    if (sl == 0) {
        ys = sy[0][r] + sy[1][r] + sy[2][r] + sy[3][r];
        ws = sw[0][r] + sw[1][r] + sw[2][r] + sw[3][r];
        y[(int64_t)gt * npad + i] = ys;
        w[(int64_t)gt * npad + i] = ws;
        const uint64_t key = (gt / T) ? key1 : key0;
        const int64_t v = i < n ? (int64_t)sdpsr_check_vector(sdpsr_check_vector_key(key), (uint32_t)i) : 0;
        const __int128 e = (__int128)ys * (__int128)ys - (__int128)v * (__int128)ws;  // |y| < 2^38, |v w| < 2^76
        const unsigned __int128 tot = check_wave_sum128((unsigned __int128)e);  // (sl == 0 is exactly the first wave)
        if (r == 0) {
            esum[((int64_t)gt * nb + blockIdx.x) * 2] = (uint64_t)tot;
            esum[((int64_t)gt * nb + blockIdx.x) * 2 + 1] = (uint64_t)(tot >> 64);
        }
    }
}

// one workgroup of G T waves; wave gt adds the nb sums of its (round, channel), a lane every 64th: |X_t v|^2 == v'C_t v exactly when
// the total is 0
__global__ void __launch_bounds__(512)
square_check_verdict_kernel(int nb, int GT, int T, const uint64_t* __restrict__ esum, uint32_t* __restrict__ bits, uint32_t* __restrict__ flag0,
                            uint32_t* __restrict__ flag1) {
    const int gt = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (gt >= GT) return;
    unsigned __int128 tot = 0;
    for (int b = lane; b < nb; b += 64) tot += ((unsigned __int128)esum[((int64_t)gt * nb + b) * 2 + 1] << 64) | (unsigned __int128)esum[((int64_t)gt * nb + b) * 2];
    tot = check_wave_sum128(tot);
    if (lane != 0) return;
    const bool differs = tot != 0;
    bits[gt] = differs ? 0u : 1u;
    if (differs) (gt / T ? flag1 : flag0)[0] = 1u;
}

template <typename LT>
void square_check_front(hipStream_t s, const SquareCheck& q, const LT* Lp) {
    const int n = (int)q.n, d = (int)q.d, nb = (int)((q.n + CHECK_TILE - 1) / CHECK_TILE);
    const uint64_t k0 = q.key[0], k1 = q.G > 1 ? q.key[1] : 0;
    const dim3 gr((unsigned)d), gp((unsigned)nb, (unsigned)nb);
    if (q.T == 2) square_check_ref_kernel<2, LT><<<gr, REF_THREADS, 0, s>>>(n, d, q.G, Lp, q.first_idx, k0, k1, q.c);
    else square_check_ref_kernel<4, LT><<<gr, REF_THREADS, 0, s>>>(n, d, q.G, Lp, q.first_idx, k0, k1, q.c);
#define SDPSR_CHECK_PASS_CASE(GG, TT)                                                                                                          \
    if (q.G == GG && q.T == TT) {                                                                                                              \
        if (q.Lfull) square_check_pass_kernel<GG, TT, true, LT><<<gp, 256, 0, s>>>(n, d, Lp, k0, k1, q.c, q.Lfull, q.part_x, q.part_c);        \
        else square_check_pass_kernel<GG, TT, false, LT><<<gp, 256, 0, s>>>(n, d, Lp, k0, k1, q.c, nullptr, q.part_x, q.part_c);               \
    }
    SDPSR_CHECK_PASS_CASE(1, 2)
    SDPSR_CHECK_PASS_CASE(1, 4)
    SDPSR_CHECK_PASS_CASE(2, 2)
    SDPSR_CHECK_PASS_CASE(2, 4)
#undef SDPSR_CHECK_PASS_CASE
}
}  // namespace

bool square_check_supports(int64_t n, int64_t d, int G, int T) {
    return n >= 1 && n <= SQUARE_CHECK_MAX_ORDER && d >= 1 && d <= SQUARE_CHECK_MAX_CLASSES && (G == 1 || G == 2) && (T == 2 || T == 4);
}
// c | part_x | part_c | y | w | esum | bits, each aligned to 16 bytes
size_t square_check_ws_bytes(int64_t n, int64_t d, int G, int T) {
    SquareCheck q;
    q.n = n, q.d = d, q.G = G, q.T = T;
    return square_check_ws_carve(q, nullptr, 0);
}
size_t square_check_ws_carve(SquareCheck& q, void* ws, size_t gap) {
    const size_t GT = (size_t)q.G * q.T, nb = (size_t)((q.n + CHECK_TILE - 1) / CHECK_TILE), npad = nb * CHECK_TILE;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        off += gap;
        char* p = ws ? (char*)ws + off : nullptr;
        off += (bytes + 15) / 16 * 16;
        return (void*)p;
    };
    q.c = (int32_t*)take(GT * (size_t)q.d * 4);
    q.part_x = (int32_t*)take(GT * nb * npad * 4);
    q.part_c = (int64_t*)take(GT * nb * npad * 8);
    q.y = (int64_t*)take(GT * npad * 8);
    q.w = (int64_t*)take(GT * npad * 8);
    q.esum = (uint64_t*)take(GT * nb * 16);
    q.bits = (uint32_t*)take(GT * 4);
    return off + gap;
}

void launch_square_check_ref_and_pass(hipStream_t s, const SquareCheck& q) {
    if (q.Lp8) square_check_front(s, q, q.Lp8);
    else square_check_front(s, q, q.Lp);
}
void launch_square_check_verdict(hipStream_t s, const SquareCheck& q) {
    const int nb = (int)((q.n + CHECK_TILE - 1) / CHECK_TILE), GT = q.G * q.T;
    const uint64_t k0 = q.key[0], k1 = q.G > 1 ? q.key[1] : 0;
    square_check_rows_kernel<<<dim3((unsigned)nb, (unsigned)GT), 256, 0, s>>>((int)q.n, nb, q.T, k0, k1, q.part_x, q.part_c, q.y, q.w, q.esum);
    square_check_verdict_kernel<<<1, 64 * GT, 0, s>>>(nb, GT, q.T, q.esum, q.bits, q.flag[0], q.G > 1 ? q.flag[1] : q.flag[0]);
}

}  // namespace sdpsr
