// Label arrays in the reference's own widths across the ABI: Partition{T} with T = UInt8 / UInt16 / UInt32
// (src/partitions.jl:6-11; admissible_subspace defaults to UInt16, :84).  sdpsr_set_label_width names the width of every label
// array the ctx's entry points read or write; inside, labels stay uint32.  The helpers below are what the entry points call in
// place of in_dev / out_dev / out_finish for a label array, and sdpsr_labels_convert is the conversion pass on its own.
#include "host_internal.h"

using namespace sdpsr;

namespace {

bool valid_width(int bits) { return bits == 8 || bits == 16 || bits == 32; }

// the flag word of the narrowing pass: pinned host memory, cleared here -- its last verdict has been read, every entry point
// returns with the stream waited for
uint32_t* narrow_flag(sdpsr_ctx* c) {
    if (!c->pinned_small) return nullptr;
    uint32_t* f = c->pinned_small + PINNED_SMALL_NARROW.first;
    *f = 0;
    return f;
}

bool element_aligned(const void* p, int bits) { return ((uintptr_t)p & (uintptr_t)(bits / 8 - 1)) == 0; }

}  // namespace

namespace sdpsr {

bool label_width_overflows(const sdpsr_ctx* c, uint64_t classes) {
    return c->label_width < 32 && classes > ((uint64_t(1) << c->label_width) - 1);
}

int label_width_fail(sdpsr_ctx* c, const char* where, uint64_t classes) {
    return ctx_fail(c, SDPSR_LABEL_OVERFLOW, std::string(where) + ": " + std::to_string(classes) + " classes do not fit the ctx's " +
                                                 std::to_string(c->label_width) + "-bit labels (sdpsr_set_label_width; InexactError of Partition{T} in the reference)");
}

int labels_fetch(sdpsr_ctx* c, uint32_t* dst32, const uint32_t* p, size_t count, int mem) {
    const int B = c->label_width;
    if (B == 32) {
        HIP_TRY(c, hipMemcpyAsync(dst32, p, count * 4, mem == SDPSR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        if (mem != SDPSR_MEM_DEVICE) c->h2d_bytes += count * 4;
        return SDPSR_OK;
    }
    const size_t bytes = count * (size_t)(B / 8);
    const void* src = p;
    if (mem != SDPSR_MEM_DEVICE) {
        void* stage = ctx_buf(c, "lab_stage", bytes);
        if (!stage) return SDPSR_OUT_OF_MEMORY;
        HIP_TRY(c, hipMemcpyAsync(stage, p, bytes, hipMemcpyHostToDevice, c->stream));
        c->h2d_bytes += bytes;
        src = stage;
    } else if (!element_aligned(p, B)) {
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "a label array is not aligned to its element");
    }
    launch_labels_widen(c->stream, (int64_t)count, src, B, dst32, c->num_cus);
    HIP_TRY(c, hipGetLastError());
    return SDPSR_OK;
}

int labels_deliver(sdpsr_ctx* c, uint32_t* p, const uint32_t* src32, size_t count, int mem) {
    const int B = c->label_width;
    if (B == 32) {
        HIP_TRY(c, hipMemcpyAsync(p, src32, count * 4, mem == SDPSR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        if (mem != SDPSR_MEM_DEVICE) c->d2h_bytes += count * 4;
        return SDPSR_OK;
    }
    const size_t bytes = count * (size_t)(B / 8);
    uint32_t* flag = narrow_flag(c);
    if (!flag) return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "pinned flag words");
    if (mem == SDPSR_MEM_DEVICE) {
        if (!element_aligned(p, B)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "a label array is not aligned to its element");
        launch_labels_narrow(c->stream, (int64_t)count, src32, p, B, flag, c->num_cus);
        HIP_TRY(c, hipGetLastError());
        return SDPSR_OK;
    }
    void* stage = ctx_buf(c, "lab_stage", bytes);
    if (!stage) return SDPSR_OUT_OF_MEMORY;
    launch_labels_narrow(c->stream, (int64_t)count, src32, stage, B, flag, c->num_cus);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(p, stage, bytes, hipMemcpyDeviceToHost, c->stream));
    c->d2h_bytes += bytes;
    return SDPSR_OK;
}

int labels_delivered(sdpsr_ctx* c) {
    if (c->label_width < 32 && c->pinned_small && c->pinned_small[PINNED_SMALL_NARROW.first])
        return ctx_fail(c, SDPSR_LABEL_OVERFLOW, "a label does not fit the ctx's " + std::to_string(c->label_width) + "-bit labels");
    return SDPSR_OK;
}

const uint32_t* labels_in_dev(sdpsr_ctx* c, const char* name, const uint32_t* p, size_t count, int mem, int* st) {
    if (c->label_width == 32) return in_dev(c, name, p, count, mem, st);
    if (!p) return p;
    uint32_t* d = (uint32_t*)ctx_buf(c, name, count * 4);
    if (!d) {
        *st = SDPSR_OUT_OF_MEMORY;
        return nullptr;
    }
    const int s = labels_fetch(c, d, p, count, mem);
    if (s) {
        *st = s;
        return nullptr;
    }
    return d;
}

uint32_t* labels_out_dev(sdpsr_ctx* c, const char* name, uint32_t* p, size_t count, int mem, int* st) {
    if (c->label_width == 32) return out_dev(c, name, p, count, mem, st);
    uint32_t* d = (uint32_t*)ctx_buf(c, name, count * 4);
    if (!d) *st = SDPSR_OUT_OF_MEMORY;
    return d;
}

int labels_out_finish(sdpsr_ctx* c, uint32_t* p, const uint32_t* dev, size_t count, int mem) {
    if (c->label_width == 32) return out_finish(c, p, dev, count, mem);
    const int st = labels_deliver(c, p, dev, count, mem);
    if (st) return st;
    HIP_TRY(c, ctx_sync_stream(c, c->stream));
    return labels_delivered(c);
}

}  // namespace sdpsr

extern "C" {

int sdpsr_set_label_width(sdpsr_ctx* c, int bits) {
    if (!c) return SDPSR_BAD_ARGUMENT;
    if (!valid_width(bits)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "label width must be 8, 16 or 32");
    c->label_width = bits;
    return SDPSR_OK;
}

int sdpsr_label_width(sdpsr_ctx* c) { return c ? c->label_width : SDPSR_BAD_ARGUMENT; }

int sdpsr_labels_convert(sdpsr_ctx* c, int64_t len, const void* in, int in_bits, void* out, int out_bits, int mem) {
    CHECK_CTX(c);
    if (!in || !out || len < 0 || !valid_width(in_bits) || !valid_width(out_bits)) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    if (len == 0) return SDPSR_OK;
    const size_t ib = (size_t)len * (in_bits / 8), ob = (size_t)len * (out_bits / 8);
    if ((const char*)in < (const char*)out + ob && (const char*)out < (const char*)in + ib)
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "labels_convert: in and out overlap");
    hipStream_t s = c->stream;
    const bool host = mem != SDPSR_MEM_DEVICE;
    if (!host && (!element_aligned(in, in_bits) || !element_aligned(out, out_bits)))
        return ctx_fail(c, SDPSR_BAD_ARGUMENT, "a label array is not aligned to its element");
    // host arrays: in travels to "conv_in" at its own width, out comes back from "conv_out" at its own
    const void* din = in;
    void* dout = out;
    if (host) {
        void* bi = ctx_buf(c, "conv_in", ib);
        dout = ctx_buf(c, "conv_out", ob);
        if (!bi || !dout) return SDPSR_OUT_OF_MEMORY;
        HIP_TRY(c, hipMemcpyAsync(bi, in, ib, hipMemcpyHostToDevice, s));
        c->h2d_bytes += ib;
        din = bi;
    }
    uint32_t* flag = narrow_flag(c);
    if (!flag) return ctx_fail(c, SDPSR_OUT_OF_MEMORY, "pinned flag words");
    if (in_bits == out_bits) {
        HIP_TRY(c, hipMemcpyAsync(dout, din, ib, hipMemcpyDeviceToDevice, s));
    } else if (in_bits == 32) {
        launch_labels_narrow(s, len, (const uint32_t*)din, dout, out_bits, flag, c->num_cus);
    } else if (out_bits == 32) {
        launch_labels_widen(s, len, din, in_bits, (uint32_t*)dout, c->num_cus);
    } else {  // 16 <-> 8: through uint32
        uint32_t* mid = (uint32_t*)ctx_buf(c, "conv_mid", (size_t)len * 4);
        if (!mid) return SDPSR_OUT_OF_MEMORY;
        launch_labels_widen(s, len, din, in_bits, mid, c->num_cus);
        launch_labels_narrow(s, len, mid, dout, out_bits, flag, c->num_cus);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, ctx_sync_stream(c, s));
    if (*flag)
        return ctx_fail(c, SDPSR_LABEL_OVERFLOW, "labels_convert: a label does not fit " + std::to_string(out_bits) + " bits (InexactError in the reference)");
    if (host) {  // (after the verdict: an overflow leaves the caller's array as it was)
        HIP_TRY(c, hipMemcpyAsync(out, dout, ob, hipMemcpyDeviceToHost, s));
        c->d2h_bytes += ob;
        HIP_TRY(c, ctx_sync_stream(c, s));
    }
    return SDPSR_OK;
}

}  // extern "C"
