// Runtime plumbing of the C ABI (include/rcfm.h): last error, version, devices, memory and streams, the placement
// arenas (rcfm_arena_*) and the host ingest (rcfm_host_register, rcfm_feeder_*).

#include <memory>
#include <mutex>
#include <set>
#include <vector>

#include "common.h"

namespace rcfm {

namespace {
thread_local std::string g_last_error;
}

void set_last_error(const std::string& msg) { g_last_error = msg; }

// ---- arena (common.h; rcfm_arena_* below) ---------------------------------------------------------------------------
}  // namespace rcfm
struct rcfm_arena_s {
    std::mutex mu;
    size_t block_bytes = 0;                 // size of a block (a request larger than that gets a block of its own size)
    struct Block {
        char* base;
        size_t bytes, used;
        bool owned;                         // false: the caller's memory (rcfm_arena_adopt)
    };
    std::vector<Block> blocks;
    size_t live = 0;                        // pieces handed out and not yet dropped
    size_t handles = 0;                     // tuner / demodulator handles created inside (they keep the pointer for life,
                                            // whether or not they hold a piece at the moment)
    ~rcfm_arena_s() {
        for (auto& b : blocks)
            if (b.owned) (void)hipFree(b.base);
    }
};
namespace rcfm {

namespace {
// Two thread-local notions, on purpose apart: what the HOST bound (rcfm_arena_bind) is only ever read when a tuner or
// demodulator handle is created; what an allocation draws from is the arena of the handle whose entry point is running
// (ArenaScope).  Function-static scratch, plan caches and the resampler / feeder handles therefore never take a piece,
// whatever is bound when they happen to allocate.
thread_local Arena* g_bound = nullptr;
thread_local Arena* g_scope = nullptr;
constexpr size_t kArenaAlign = (size_t)2 << 20;   // pieces start on 2 MiB boundaries (the large-page size)
std::mutex g_arenas_mu;
std::set<Arena*> g_arenas;                        // arenas that exist (a binding left behind on another thread is checked)

// A new arena joins the set of live ones and goes to the caller.
Arena* arena_register(std::unique_ptr<Arena> a) {
    std::lock_guard<std::mutex> reg(g_arenas_mu);
    g_arenas.insert(a.get());
    return a.release();
}
}  // namespace

Arena* current_arena() { return g_scope; }

Arena* arena_enter_handle() {
    Arena* a = g_bound;
    if (!a) return nullptr;
    std::lock_guard<std::mutex> reg(g_arenas_mu);
    if (!g_arenas.count(a)) {   // destroyed on another thread while still bound here
        g_bound = nullptr;
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(a->mu);
    a->handles += 1;
    return a;
}

void arena_leave_handle(Arena* a) {
    if (!a) return;
    std::lock_guard<std::mutex> lock(a->mu);
    if (a->handles) a->handles -= 1;
}

void* arena_take(Arena* a, size_t bytes) {
    std::lock_guard<std::mutex> lock(a->mu);
    const size_t need = (bytes + kArenaAlign - 1) / kArenaAlign * kArenaAlign;
    for (auto& b : a->blocks)
        if (b.bytes - b.used >= need) {
            void* p = b.base + b.used;
            b.used += need;
            a->live += 1;
            return p;
        }
    void* base = nullptr;
    const size_t sz = std::max(a->block_bytes, need);
    RC_HIP(hipMalloc(&base, sz));
    a->blocks.push_back(Arena::Block{static_cast<char*>(base), sz, need, true});
    a->live += 1;
    return base;
}

void arena_drop(Arena* a) {
    std::lock_guard<std::mutex> lock(a->mu);
    if (a->live) a->live -= 1;
}

ArenaScope::ArenaScope(Arena* a) : prev(g_scope) { g_scope = a; }
ArenaScope::~ArenaScope() { g_scope = prev; }

}  // namespace rcfm

using namespace rcfm;

// Overlapped host -> device ingest (rcfm_feeder_*): `depth` device slots, one copy stream, an event pair per slot.
struct rcfm_feeder_s {
    size_t bytes = 0;
    int depth = 0;
    bool owns = false;
    std::vector<void*> slot;
    std::vector<hipEvent_t> ready, done;   // ready: the copy into the slot has landed; done: its consumer has finished
    hipStream_t copy = nullptr;
    uint64_t head = 0, tail = 0;           // submitted / released buffers
    uint64_t landed = 0;                   // buffers whose copy is known to have completed (rcfm_feeder_copied)
    ~rcfm_feeder_s() {
        if (copy) (void)hipStreamSynchronize(copy);
        for (auto e : ready) (void)hipEventDestroy(e);
        for (auto e : done) (void)hipEventDestroy(e);
        if (owns)
            for (auto p : slot) (void)hipFree(p);
        if (copy) (void)hipStreamDestroy(copy);
    }
};

extern "C" {

int rcfm_version(void) { return RCFM_VERSION; }

const char* rcfm_last_error(void) { return g_last_error.c_str(); }

int rcfm_device_count(int* count) {
    return guarded([&] {
        RC_REQUIRE(count != nullptr, RCFM_ERR_ARG, "count is NULL");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        *count = (e == hipSuccess) ? n : 0;
        if (e != hipSuccess) (void)hipGetLastError();
    });
}

int rcfm_malloc(void** dptr, size_t bytes) {
    return guarded([&] {
        RC_REQUIRE(dptr != nullptr, RCFM_ERR_ARG, "dptr is NULL");
        RC_HIP(hipMalloc(dptr, bytes));
    });
}

int rcfm_free(void* dptr) {
    return guarded([&] { RC_HIP(hipFree(dptr)); });
}

int rcfm_memcpy_h2d(void* dst, const void* src_host, size_t bytes, void* stream) {
    return guarded([&] { RC_HIP(hipMemcpyAsync(dst, src_host, bytes, hipMemcpyHostToDevice, as_stream(stream))); });
}

int rcfm_memcpy_d2h(void* dst_host, const void* src, size_t bytes, void* stream) {
    return guarded([&] { RC_HIP(hipMemcpyAsync(dst_host, src, bytes, hipMemcpyDeviceToHost, as_stream(stream))); });
}

int rcfm_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
    return guarded([&] { RC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream))); });
}

int rcfm_stream_sync(void* stream) {
    return guarded([&] { RC_HIP(hipStreamSynchronize(as_stream(stream))); });
}

int rcfm_stream_create(void** stream) {
    return guarded([&] {
        RC_REQUIRE(stream != nullptr, RCFM_ERR_ARG, "stream is NULL");
        hipStream_t s = nullptr;
        RC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        *stream = s;
    });
}

int rcfm_stream_destroy(void* stream) {
    return guarded([&] {
        if (stream) RC_HIP(hipStreamDestroy(as_stream(stream)));
    });
}

// ---- placement -----------------------------------------------------------------

int rcfm_arena_create(size_t block_bytes, rcfm_arena_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr, RCFM_ERR_ARG, "out is NULL");
        auto a = std::make_unique<Arena>();
        a->block_bytes = block_bytes ? block_bytes : ((size_t)1 << 30);
        if (block_bytes) {   // the first block now: its placement is the draw the caller asked for
            void* base = nullptr;
            RC_HIP(hipMalloc(&base, a->block_bytes));
            a->blocks.push_back(Arena::Block{static_cast<char*>(base), a->block_bytes, 0, true});
        }
        *out = arena_register(std::move(a));
    });
}

int rcfm_arena_adopt(void* base, size_t bytes, rcfm_arena_t* out) {
    return guarded([&] {
        RC_REQUIRE(out && base && bytes >= kArenaAlign, RCFM_ERR_ARG, "bad arena memory");
        auto a = std::make_unique<Arena>();
        a->block_bytes = (size_t)1 << 30;   // what does not fit the caller's memory comes from hipMalloc in 1 GiB blocks
        char* p = static_cast<char*>(base);
        const size_t skew = (kArenaAlign - (reinterpret_cast<uintptr_t>(p) & (kArenaAlign - 1))) & (kArenaAlign - 1);
        RC_REQUIRE(bytes > skew + kArenaAlign, RCFM_ERR_ARG, "bad arena memory");
        a->blocks.push_back(Arena::Block{p + skew, (bytes - skew) / kArenaAlign * kArenaAlign, 0, false});
        *out = arena_register(std::move(a));
    });
}

int rcfm_arena_bind(rcfm_arena_t a) {
    return guarded([&] {
        if (a) {
            std::lock_guard<std::mutex> reg(g_arenas_mu);
            RC_REQUIRE(g_arenas.count(a) != 0, RCFM_ERR_ARG, "not a live arena");
        }
        g_bound = a;
    });
}

int rcfm_arena_stats(rcfm_arena_t a, size_t* reserved_bytes, size_t* used_bytes, size_t* live_pieces) {
    return guarded([&] {
        RC_REQUIRE(a != nullptr, RCFM_ERR_ARG, "NULL arena");
        std::lock_guard<std::mutex> lock(a->mu);
        size_t r = 0, u = 0;
        for (auto& b : a->blocks) {
            r += b.bytes;
            u += b.used;
        }
        if (reserved_bytes) *reserved_bytes = r;
        if (used_bytes) *used_bytes = u;
        if (live_pieces) *live_pieces = a->live;
    });
}

int rcfm_arena_destroy(rcfm_arena_t a) {
    return guarded([&] {
        if (!a) return;
        {
            std::lock_guard<std::mutex> reg(g_arenas_mu);
            RC_REQUIRE(g_arenas.count(a) != 0, RCFM_ERR_ARG, "not a live arena");
            {
                // handles, not pieces: a tuner whose spectrum was attached, or a handle of small buffers only, holds no
                // piece and still allocates from its arena on its next run
                std::lock_guard<std::mutex> lock(a->mu);
                RC_REQUIRE(a->handles == 0 && a->live == 0, RCFM_ERR_STATE,
                           "handles created inside this arena are still alive: destroy them first");
            }
            g_arenas.erase(a);   // a binding another thread still holds is dropped when that thread next creates a handle
        }
        if (g_bound == a) g_bound = nullptr;
        delete a;
    });
}

// ---- host ingest -----------------------------------------------------------------

int rcfm_host_register(void* host, size_t bytes) {
    return guarded([&] {
        RC_REQUIRE(host != nullptr && bytes > 0, RCFM_ERR_ARG, "bad host range");
        RC_HIP(hipHostRegister(host, bytes, hipHostRegisterDefault));
    });
}

int rcfm_host_unregister(void* host) {
    return guarded([&] { RC_HIP(hipHostUnregister(host)); });
}

int rcfm_feeder_create(size_t bytes, int depth, void* const* device_slots, rcfm_feeder_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr && bytes > 0 && depth >= 1 && depth <= 16, RCFM_ERR_ARG, "bad feeder geometry");
        auto f = std::make_unique<rcfm_feeder_s>();
        f->bytes = bytes;
        f->depth = depth;
        f->owns = device_slots == nullptr;
        RC_HIP(hipStreamCreateWithFlags(&f->copy, hipStreamNonBlocking));
        for (int i = 0; i < depth; ++i) {
            void* p = device_slots ? device_slots[i] : nullptr;
            if (!device_slots) RC_HIP(hipMalloc(&p, bytes));
            RC_REQUIRE(p != nullptr, RCFM_ERR_ARG, "NULL device slot");
            f->slot.push_back(p);
            hipEvent_t a, b;
            RC_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
            f->ready.push_back(a);
            RC_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
            f->done.push_back(b);
        }
        *out = f.release();
    });
}

int rcfm_feeder_submit(rcfm_feeder_t f, const void* src_host) {
    return guarded([&] {
        RC_REQUIRE(f && src_host, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(f->head - f->tail < (uint64_t)f->depth, RCFM_ERR_STATE,
                   "every feeder slot is in flight: release one before submitting another buffer");
        const int i = (int)(f->head % (uint64_t)f->depth);
        RC_HIP(hipStreamWaitEvent(f->copy, f->done[i], 0));   // the kernels that read this slot last time are finished
        RC_HIP(hipMemcpyAsync(f->slot[i], src_host, f->bytes, hipMemcpyHostToDevice, f->copy));
        RC_HIP(hipEventRecord(f->ready[i], f->copy));
        f->head += 1;
    });
}

int rcfm_feeder_acquire(rcfm_feeder_t f, void* stream, void** dptr) {
    return guarded([&] {
        RC_REQUIRE(f && dptr, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(f->tail < f->head, RCFM_ERR_STATE, "rcfm_feeder_acquire without a submitted buffer");
        const int i = (int)(f->tail % (uint64_t)f->depth);
        RC_HIP(hipStreamWaitEvent(as_stream(stream), f->ready[i], 0));
        *dptr = f->slot[i];
    });
}

int rcfm_feeder_release(rcfm_feeder_t f, void* stream) {
    return guarded([&] {
        RC_REQUIRE(f, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(f->tail < f->head, RCFM_ERR_STATE, "rcfm_feeder_release without an acquired buffer");
        const int i = (int)(f->tail % (uint64_t)f->depth);
        RC_HIP(hipEventRecord(f->done[i], as_stream(stream)));
        f->tail += 1;
    });
}

int rcfm_feeder_copied(rcfm_feeder_t f, uint64_t* count) {
    return guarded([&] {
        RC_REQUIRE(f && count, RCFM_ERR_ARG, "NULL argument");
        // Copies complete in submission order (one copy stream).  ready[i] always refers to the LATEST copy into
        // slot i; when buffer k's slot has been re-submitted since, that newer copy ran behind k on the same stream,
        // so "the newer copy is complete" still implies "k has landed", and "not ready" merely answers conservatively.
        while (f->landed < f->head) {
            const hipError_t e = hipEventQuery(f->ready[(size_t)(f->landed % (uint64_t)f->depth)]);
            if (e == hipErrorNotReady) break;
            RC_HIP(e);
            f->landed += 1;
        }
        *count = f->landed;
    });
}

int rcfm_feeder_destroy(rcfm_feeder_t f) {
    return guarded([&] { delete f; });
}

}  // extern "C"
