// Multi-GPU transport (rcfm_comm_*): the audio gather and the spectrum hand-over between ranks, over an RCCL that is
// opened on the first call.

#include <cstring>
#include <memory>
#include <mutex>
#include <string>

#include <dlfcn.h>
#include <rccl/rccl.h>   // types only: the library is opened on the first rcfm_comm_* call (dlopen), never linked

#include "common.h"

using namespace rcfm;

namespace {

// RCCL, bound at run time: a process that never gathers (one GPU, or a host that gathers with its own transport)
// does not load it; a process that already loaded an RCCL (PyTorch's ProcessGroupNCCL) gets that same copy.
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Gather)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        // a copy some other component of this process already mapped (PyTorch's ProcessGroupNCCL loads
        // torch/lib/librccl.so, SONAME librccl.so.1) is reused: two RCCL instances in one process would each
        // own a set of communicators and IPC handles
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            r.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);
            if (r.lib) break;
        }
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            if (r.lib) break;
            r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        }
        if (!r.lib) return;
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
        r.Gather = reinterpret_cast<decltype(r.Gather)>(dlsym(r.lib, "ncclGather"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
        r.Send = reinterpret_cast<decltype(r.Send)>(dlsym(r.lib, "ncclSend"));
        r.Recv = reinterpret_cast<decltype(r.Recv)>(dlsym(r.lib, "ncclRecv"));
        r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(dlsym(r.lib, "ncclGroupStart"));
        r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(dlsym(r.lib, "ncclGroupEnd"));
    });
    RC_REQUIRE(r.lib && r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.Gather && r.Send && r.Recv && r.GroupStart &&
                   r.GroupEnd,
               RCFM_ERR_RUNTIME,
               "RCCL (librccl.so) is not available in this process");
    return r;
}

}  // namespace

#define RC_NCCL(expr)                                                                              \
    do {                                                                                           \
        ncclResult_t rc_n_ = (expr);                                                               \
        if (rc_n_ != ncclSuccess)                                                                  \
            throw ::rcfm::Error{RCFM_ERR_RUNTIME, std::string(#expr) + ": " +                      \
                                                      (rccl().GetErrorString ? rccl().GetErrorString(rc_n_) : "RCCL error")}; \
    } while (0)

struct rcfm_comm_s {
    ncclComm_t comm = nullptr;
    int world = 1, rank = 0;
    int group_depth = 0;   // rcfm_comm_group_start without its rcfm_comm_group_end
};

extern "C" {

// ---- multi-GPU: the audio gather ------------------------------------------------------

int rcfm_comm_unique_id(void* id128_host) {
    return guarded([&] {
        RC_REQUIRE(id128_host != nullptr, RCFM_ERR_ARG, "NULL argument");
        static_assert(sizeof(ncclUniqueId) == RCFM_UNIQUE_ID_BYTES, "RCCL unique id size changed");
        ncclUniqueId id;
        RC_NCCL(rccl().GetUniqueId(&id));
        std::memcpy(id128_host, &id, sizeof(id));
    });
}

int rcfm_comm_init_rank(int world, int rank, const void* id128_host, rcfm_comm_t* out) {
    return guarded([&] {
        RC_REQUIRE(out && id128_host && world >= 1 && rank >= 0 && rank < world, RCFM_ERR_ARG, "bad communicator geometry");
        auto c = std::make_unique<rcfm_comm_s>();
        c->world = world;
        c->rank = rank;
        ncclUniqueId id;
        std::memcpy(&id, id128_host, sizeof(id));
        RC_NCCL(rccl().CommInitRank(&c->comm, world, id, rank));
        *out = c.release();
    });
}

int rcfm_gather_audio(rcfm_comm_t c, int root, const void* send, size_t floats_per_rank, void* recv, void* stream) {
    return guarded([&] {
        RC_REQUIRE(c && send, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(root >= 0 && root < c->world, RCFM_ERR_INDEX, "root rank outside the communicator");
        RC_REQUIRE(c->rank != root || recv != nullptr, RCFM_ERR_ARG, "the root rank needs a receive buffer");
        RC_NCCL(rccl().Gather(send, recv, floats_per_rank, ncclFloat32, root, c->comm, as_stream(stream)));
    });
}

// ---- multi-GPU: the spectrum hand-over of the rotating FFT owner -------------------------

int rcfm_comm_group_start(rcfm_comm_t c) {
    return guarded([&] {
        RC_REQUIRE(c, RCFM_ERR_ARG, "NULL communicator");
        RC_NCCL(rccl().GroupStart());
        ++c->group_depth;
    });
}

int rcfm_comm_group_end(rcfm_comm_t c) {
    return guarded([&] {
        RC_REQUIRE(c, RCFM_ERR_ARG, "NULL communicator");
        RC_REQUIRE(c->group_depth > 0, RCFM_ERR_STATE, "rcfm_comm_group_end without rcfm_comm_group_start");
        --c->group_depth;
        RC_NCCL(rccl().GroupEnd());
    });
}

int rcfm_send_bins(rcfm_comm_t c, int peer, const void* bins, size_t nbins, void* stream) {
    return guarded([&] {
        RC_REQUIRE(c && (bins || nbins == 0), RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(peer >= 0 && peer < c->world, RCFM_ERR_INDEX, "peer rank outside the communicator");
        RC_REQUIRE(peer != c->rank || c->group_depth > 0, RCFM_ERR_STATE,
                   "a transfer to this rank itself needs its receive in the same group (rcfm_comm_group_start)");
        if (nbins == 0) return;   // a rank that owns no channels reads no bins
        RC_NCCL(rccl().Send(bins, 2 * nbins, ncclFloat32, peer, c->comm, as_stream(stream)));
    });
}

int rcfm_recv_bins(rcfm_comm_t c, int peer, void* bins, size_t nbins, void* stream) {
    return guarded([&] {
        RC_REQUIRE(c && (bins || nbins == 0), RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(peer >= 0 && peer < c->world, RCFM_ERR_INDEX, "peer rank outside the communicator");
        RC_REQUIRE(peer != c->rank || c->group_depth > 0, RCFM_ERR_STATE,
                   "a transfer from this rank itself needs its send in the same group (rcfm_comm_group_start)");
        if (nbins == 0) return;
        RC_NCCL(rccl().Recv(bins, 2 * nbins, ncclFloat32, peer, c->comm, as_stream(stream)));
    });
}

int rcfm_comm_destroy(rcfm_comm_t c) {
    return guarded([&] {
        if (c && c->comm) (void)rccl().CommDestroy(c->comm);
        delete c;
    });
}

}  // extern "C"
