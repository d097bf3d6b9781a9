// The agreement of independent restarts behind the C ABI: sdpsr_meet_keys, sdpsr_agree_partitions,
// sdpsr_agree_block_diagonalization.  The decisions are agree_plan.h (plain host arithmetic), the key pass is
// kernels_agree.hip, the collectives are comm.cpp; checksum, relabel and the narrowing pass are the ones the other entry
// points use.  Reference: Base.:(==) and refine! of src/partitions.jl:16-17,62-66; the "try again" of
// src/eigen_decomposition.jl:264-270 and src/diagonalize.jl:4-9.
#include "host_internal.h"

using namespace sdpsr;

namespace {

bool element_aligned(const void* p, int bits) { return ((uintptr_t)p & (uintptr_t)(bits / 8 - 1)) == 0; }

// The caller's R arrays as device arrays at the ctx's label width: device memory as it lies, host memory uploaded into one
// staging buffer (the arrays with valid[i] == 0 are skipped: dev[i] stays nullptr).  Checks what the memory space demands.
int arrays_on_device(sdpsr_ctx* c, int32_t R, const uint32_t* const* labels, const int32_t* valid, int64_t len, int mem,
                     const void** dev) {
    const int B = c->label_width;
    const size_t bytes = (size_t)len * (size_t)(B / 8), pitch = (bytes + 15) & ~size_t(15);
    char* stage = nullptr;
    if (mem != SDPSR_MEM_DEVICE) {
        stage = (char*)ctx_buf(c, "agree_in", pitch * (size_t)R);
        if (!stage) return SDPSR_OUT_OF_MEMORY;
    }
    for (int32_t i = 0; i < R; ++i) {
        dev[i] = nullptr;
        if (mem == SDPSR_MEM_DEVICE && !element_aligned(labels[i], B))  // (an invalid restart's too: the meet is delivered into it)
            return ctx_fail(c, SDPSR_BAD_ARGUMENT, "a label array is not aligned to its element");
        if (valid && !valid[i]) continue;
        if (mem == SDPSR_MEM_DEVICE) {
            dev[i] = labels[i];
        } else {
            HIP_TRY(c, hipMemcpyAsync(stage + pitch * (size_t)i, labels[i], bytes, hipMemcpyHostToDevice, c->stream));
            c->h2d_bytes += bytes;
            dev[i] = stage + pitch * (size_t)i;
        }
    }
    return SDPSR_OK;
}

// the key pass over the arrays that are there (dev[i] != nullptr), slot first_slot + i for array i
int meet_keys_device(sdpsr_ctx* c, int32_t R, const void* const* dev, int64_t len, int64_t first_slot, uint64_t* keys) {
    const void* arr[AGREE_MAX_RESTARTS];
    uint64_t mult[AGREE_MAX_RESTARTS];
    int nv = 0;
    for (int32_t i = 0; i < R; ++i)
        if (dev[i]) {
            arr[nv] = dev[i];
            mult[nv++] = agree_multiplier((uint64_t)(first_slot + i));
        }
    launch_meet_keys(c->stream, len, nv, arr, mult, c->label_width, keys, c->num_cus);
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

int check_restarts(sdpsr_ctx* c, int32_t R, const uint32_t* const* labels, int64_t len) {
    if (R < 1 || R > AGREE_MAX_RESTARTS) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "R out of range [1, 64]");
    if (!labels) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    for (int32_t i = 0; i < R; ++i)
        if (!labels[i]) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    return check_len(c, len);
}

}  // namespace

extern "C" {

int sdpsr_meet_keys(sdpsr_ctx* c, int32_t R, const uint32_t* const* labels, const int32_t* valid, int64_t len, int64_t first_slot,
                    uint64_t* keys, int mem) {
    CHECK_CTX(c);
    int st = check_restarts(c, R, labels, len);
    if (st) return st;
    if (!keys || first_slot < 0) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null keys or a negative first_slot");
    if (mem == SDPSR_MEM_DEVICE && ((uintptr_t)keys & 7u)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "keys is not aligned to 8 bytes");
    const void* dev[AGREE_MAX_RESTARTS];
    st = arrays_on_device(c, R, labels, valid, len, mem, dev);
    if (st) return st;
    uint64_t* dK = out_dev(c, "agree_keys", keys, (size_t)len, mem, &st);
    if (st) return st;
    st = meet_keys_device(c, R, dev, len, first_slot, dK);
    if (st) return st;
    return out_finish(c, keys, dK, (size_t)len, mem);
}

int sdpsr_agree_partitions(sdpsr_ctx* c, sdpsr_comm* comm, int32_t R, uint32_t* const* labels, const int32_t* valid, int64_t len,
                           int64_t* dim_out, int32_t* met, int mem) {
    CHECK_CTX(c);
    int st = check_restarts(c, R, labels, len);
    if (st) return st;
    if (!dim_out || !met) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    if (comm && (st = comm_usable(c, comm))) return st;
    const int B = c->label_width;
    const void* dev[AGREE_MAX_RESTARTS];
    st = arrays_on_device(c, R, labels, valid, len, mem, dev);
    if (st) return st;

    // 1. the checksums of the valid restarts, one read-back
    uint64_t* words = (uint64_t*)ctx_buf(c, "agree_words", (size_t)2 * AGREE_MAX_RESTARTS * 8);
    uint64_t* scratch = (uint64_t*)ctx_buf(c, "chk_scratch", (size_t)(2 * 2048 + 2) * 8);
    uint32_t* wide = B == 32 ? nullptr : (uint32_t*)ctx_buf(c, "agree_w32", (size_t)len * 4);
    if (!words || !scratch || (B != 32 && !wide)) return SDPSR_OUT_OF_MEMORY;
    HIP_TRY(c, hipMemsetAsync(words, 0, (size_t)2 * R * 8, c->stream));
    for (int32_t i = 0; i < R; ++i) {
        if (!dev[i]) continue;
        const uint32_t* L32 = (const uint32_t*)dev[i];
        if (B != 32) {  // (the checksum kernel reads uint32; the arrays themselves stay as they are for the key pass)
            launch_labels_widen(c->stream, len, dev[i], B, wide, c->num_cus);
            L32 = wide;
        }
        launch_labels_checksum(c->stream, len, L32, scratch, words + 2 * i);
    }
    HIP_TRY(c, hipGetLastError());
    uint64_t hw[2 * AGREE_MAX_RESTARTS];
    st = d2h_sync(c, hw, words, (size_t)2 * R * 8);
    if (st) return st;

    // 2. the table and the decision every rank takes from it
    AgreeRecord mine;
    mine.len = len;
    mine.R = R;
    mine.width = B;
    for (int32_t i = 0; i < R; ++i) {
        mine.valid[i] = dev[i] ? 1 : 0;
        mine.word0[i] = hw[2 * i];
        mine.word1[i] = hw[2 * i + 1];
    }
    const int32_t world = comm ? comm->world : 1, rank = comm ? comm->rank : 0;
    std::vector<AgreeRecord> table((size_t)world);
    if (comm) {
        st = comm_all_gather(c, comm, &mine, sizeof(AgreeRecord), table.data());
        if (st) return st;
    } else {
        table[0] = mine;
    }
    switch (agree_plan(world, table.data())) {
        case AGREE_MISMATCH: return ctx_fail(c, SDPSR_BAD_ARGUMENT, "agree_partitions: the ranks disagree on len, R or the label width");
        case AGREE_NONE_VALID: return ctx_fail(c, SDPSR_BAD_STATE, "agree_partitions: no valid restart on any rank");
        case AGREE_AGREED: *met = 0; return SDPSR_OK;
        case AGREE_MEET: break;
    }

    // 3. the meet: key pass, one all-reduce, canonical relabel, delivered into every array
    uint64_t* keys = (uint64_t*)ctx_buf(c, "agree_keys", (size_t)len * 8);
    uint64_t* sig = (uint64_t*)ctx_buf(c, "sig", (size_t)len * 8);
    uint32_t* dL = (uint32_t*)ctx_buf(c, "prim_out", (size_t)len * 4);
    if (!keys || !sig || !dL) return SDPSR_OUT_OF_MEMORY;
    st = meet_keys_device(c, R, dev, len, agree_first_slot(rank, R), keys);
    if (st) return st;
    if (comm && (st = comm_all_reduce_sum_u64(c, comm, keys, len))) return st;
    launch_sig_u64(c->stream, len, keys, sig);
    int64_t nparts = 0;
    st = refine_signatures(c, len, sig, dL, &nparts);
    if (st) return st;
    *dim_out = nparts;
    if (label_overflows(c, (uint64_t)nparts)) return label_overflow_fail(c, "agree_partitions", (uint64_t)nparts);
    if (label_width_overflows(c, (uint64_t)nparts)) return label_width_fail(c, "agree_partitions", (uint64_t)nparts);  // (arrays untouched)
    for (int32_t i = 0; i < R; ++i) {
        st = labels_deliver(c, labels[i], dL, (size_t)len, mem);
        if (st) return st;
    }
    HIP_TRY(c, ctx_sync_stream(c, c->stream));
    st = labels_delivered(c);
    if (st) return st;
    *met = 1;
    return SDPSR_OK;
}

int sdpsr_agree_block_diagonalization(sdpsr_ctx* c, sdpsr_comm* comm, int32_t status, int32_t nblocks, const int32_t* blk_sizes,
                                      int32_t* winner, int32_t* nblocks_out, int32_t* sizes_out, int32_t capacity) {
    CHECK_CTX(c);
    if (!winner || !nblocks_out || capacity < 0 || (capacity > 0 && !sizes_out) || (status == SDPSR_OK && (nblocks < 0 || (nblocks > 0 && !blk_sizes))))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    int st = SDPSR_OK;
    if (comm && (st = comm_usable(c, comm))) return st;
    const int32_t world = comm ? comm->world : 1, rank = comm ? comm->rank : 0;
    const int32_t mine[2] = {status, status == SDPSR_OK ? nblocks : 0};
    std::vector<int32_t> table((size_t)2 * world), statuses((size_t)world);
    if (comm) {
        st = comm_all_gather(c, comm, mine, sizeof(mine), table.data());
        if (st) return st;
    } else {
        table[0] = mine[0];
        table[1] = mine[1];
    }
    for (int32_t r = 0; r < world; ++r) statuses[r] = table[2 * r];
    const int32_t w = agree_winner(world, statuses.data());
    *winner = w;
    *nblocks_out = w < 0 ? 0 : table[2 * w + 1];
    if (w < 0 || *nblocks_out == 0) return SDPSR_OK;
    const int32_t nb = *nblocks_out;
    std::vector<int32_t> sizes((size_t)nb);
    if (comm) {  // (every rank takes part, whatever its capacity: the ranks stay in step)
        int32_t* d = (int32_t*)ctx_buf(c, "comm_sizes", (size_t)nb * 4);
        if (!d) return SDPSR_OUT_OF_MEMORY;
        if (rank == w && (st = h2d_sync(c, d, blk_sizes, (size_t)nb * 4))) return st;
        st = comm_broadcast_dev(c, comm, d, (size_t)nb * 4, w);
        if (st) return st;
        st = d2h_sync(c, sizes.data(), d, (size_t)nb * 4);
        if (st) return st;
    } else {
        std::copy(blk_sizes, blk_sizes + nb, sizes.begin());
    }
    if (nb > capacity) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "agree_block_diagonalization: " + std::to_string(nb) + " block sizes do not fit the capacity");
    std::copy(sizes.begin(), sizes.end(), sizes_out);
    return SDPSR_OK;
}

}  // extern "C"
