// The communicator of include/sdpsr.h: RCCL behind the C ABI, one process per GPU.  RCCL is opened on the first sdpsr_comm_*
// call with dlopen("librccl.so.1") -- by SONAME: the library does not link against it, and a process that has imported torch
// shares the RCCL torch has mapped (the arrangement of DESIGN 6 for libamdhip64).  Only the types come from <rccl/rccl.h>.
// Every collective runs on the ctx's stream; the library adds no time-out of its own.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "host_internal.h"

using namespace sdpsr;

namespace {

struct RcclApi {
    std::string err;  // empty: every pointer below is set
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

RcclApi open_rccl() {
    RcclApi a;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        const char* e = dlerror();
        a.err = std::string("dlopen(librccl.so.1): ") + (e ? e : "unknown error");
        return a;
    }
    auto sym = [&](const char* name) -> void* {
        void* p = dlsym(h, name);
        if (!p && a.err.empty()) {
            const char* e = dlerror();
            a.err = std::string("librccl.so.1 lacks ") + name + (e ? std::string(": ") + e : std::string());
        }
        return p;
    };
    a.GetUniqueId = (decltype(a.GetUniqueId))sym("ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))sym("ncclCommInitRank");
    a.AllGather = (decltype(a.AllGather))sym("ncclAllGather");
    a.AllReduce = (decltype(a.AllReduce))sym("ncclAllReduce");
    a.Broadcast = (decltype(a.Broadcast))sym("ncclBroadcast");
    a.CommDestroy = (decltype(a.CommDestroy))sym("ncclCommDestroy");
    a.GetErrorString = (decltype(a.GetErrorString))sym("ncclGetErrorString");
    return a;  // (the handle stays open for the life of the process)
}

// opened once per process, on first use (thread-safe: a function-local static); a failure is remembered
const RcclApi& rccl() {
    static const RcclApi api = open_rccl();
    return api;
}

int rccl_unavailable(sdpsr_ctx* c) { return ctx_fail(c, SDPSR_BAD_STATE, rccl().err); }
int rccl_fail(sdpsr_ctx* c, const char* what, ncclResult_t r) {
    return ctx_fail(c, SDPSR_SOLVER_ERROR, std::string(what) + ": " + rccl().GetErrorString(r));
}

#define RCCL_TRY(c, what, expr)                                     \
    do {                                                            \
        const ncclResult_t _r = (expr);                             \
        if (_r != ncclSuccess) return rccl_fail((c), (what), _r);   \
    } while (0)

}  // namespace

namespace sdpsr {

int comm_usable(sdpsr_ctx* c, const sdpsr_comm* comm) {
    if (!comm->nccl || comm->device != c->device) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "the communicator was not created on this ctx's device");
    return SDPSR_OK;
}

int comm_all_gather(sdpsr_ctx* c, sdpsr_comm* comm, const void* mine, size_t bytes, void* table) {
    char* send = (char*)ctx_buf(c, "comm_send", bytes);
    char* recv = (char*)ctx_buf(c, "comm_recv", bytes * (size_t)comm->world);
    if (!send || !recv) return SDPSR_OUT_OF_MEMORY;
    int st = h2d_sync(c, send, mine, bytes);
    if (st) return st;
    RCCL_TRY(c, "ncclAllGather", rccl().AllGather(send, recv, bytes, ncclChar, (ncclComm_t)comm->nccl, c->stream));
    return d2h_sync(c, table, recv, bytes * (size_t)comm->world);
}

int comm_all_reduce_sum_u64(sdpsr_ctx* c, sdpsr_comm* comm, uint64_t* dev, int64_t count) {
    RCCL_TRY(c, "ncclAllReduce", rccl().AllReduce(dev, dev, (size_t)count, ncclUint64, ncclSum, (ncclComm_t)comm->nccl, c->stream));
    return SDPSR_OK;
}

int comm_broadcast_dev(sdpsr_ctx* c, sdpsr_comm* comm, void* dev, size_t bytes, int32_t root) {
    RCCL_TRY(c, "ncclBroadcast", rccl().Broadcast(dev, dev, bytes, ncclChar, root, (ncclComm_t)comm->nccl, c->stream));
    return SDPSR_OK;
}

}  // namespace sdpsr

extern "C" {

int sdpsr_comm_unique_id(void* id128) {
    static_assert(sizeof(ncclUniqueId) == 128, "the header promises 128 bytes");
    if (!id128) return SDPSR_BAD_ARGUMENT;
    if (!rccl().err.empty()) return SDPSR_BAD_STATE;  // (no ctx to carry the message: sdpsr_comm_create repeats it)
    ncclUniqueId id;
    if (rccl().GetUniqueId(&id) != ncclSuccess) return SDPSR_SOLVER_ERROR;
    memcpy(id128, &id, sizeof(id));
    return SDPSR_OK;
}

int sdpsr_comm_create(sdpsr_ctx* c, int32_t world, int32_t rank, const void* id128, sdpsr_comm** out) {
    CHECK_CTX(c);
    if (!out) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "null pointer");
    *out = nullptr;
    if (!id128 || world < 1 || rank < 0 || rank >= world) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    if (!rccl().err.empty()) return rccl_unavailable(c);
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t nc = nullptr;
    RCCL_TRY(c, "ncclCommInitRank", rccl().CommInitRank(&nc, world, id, rank));  // (on the current device: ctx's, CHECK_CTX)
    sdpsr_comm* comm = new sdpsr_comm();
    comm->device = c->device;
    comm->world = world;
    comm->rank = rank;
    comm->nccl = nc;
    *out = comm;
    return SDPSR_OK;
}

int sdpsr_comm_rank(const sdpsr_comm* comm) { return comm ? comm->rank : -1; }
int sdpsr_comm_world(const sdpsr_comm* comm) { return comm ? comm->world : -1; }

int sdpsr_comm_broadcast(sdpsr_ctx* c, sdpsr_comm* comm, void* buf, int64_t bytes, int32_t root, int mem) {
    CHECK_CTX(c);
    if (!comm || !buf || bytes < 0 || root < 0 || root >= comm->world) return ctx_fail(c, SDPSR_BAD_ARGUMENT, "bad arguments");
    int st = comm_usable(c, comm);
    if (st) return st;
    if (bytes == 0) return SDPSR_OK;
    void* d = buf;
    if (mem != SDPSR_MEM_DEVICE) {
        d = ctx_buf(c, "comm_bcast", (size_t)bytes);
        if (!d) return SDPSR_OUT_OF_MEMORY;
        if (comm->rank == root) {
            HIP_TRY(c, hipMemcpyAsync(d, buf, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
            c->h2d_bytes += (uint64_t)bytes;
        }
    }
    st = comm_broadcast_dev(c, comm, d, (size_t)bytes, root);
    if (st) return st;
    if (mem != SDPSR_MEM_DEVICE && comm->rank != root) {
        HIP_TRY(c, hipMemcpyAsync(buf, d, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
        c->d2h_bytes += (uint64_t)bytes;
    }
    HIP_TRY(c, ctx_sync_stream(c, c->stream));
    return SDPSR_OK;
}

int sdpsr_comm_destroy(sdpsr_comm* comm) {
    if (!comm) return SDPSR_BAD_ARGUMENT;
    int st = SDPSR_OK;
    if (comm->nccl) {
        DeviceGuard dg(comm->device);
        if (rccl().CommDestroy((ncclComm_t)comm->nccl) != ncclSuccess) st = SDPSR_SOLVER_ERROR;
    }
    delete comm;
    return st;
}

}  // extern "C"
