// Audio egress (include/rcfm.h, "audio egress" and "host egress"): rcfm_audio_pack packs the open channels' audio densely as
// int16 PCM (or float32 unchanged), and rcfm_drain_* moves header and payload to page-locked host memory on two copy
// streams, behind the next buffer's kernels.  The mirror of the host ingest (runtime.hip, rcfm_feeder_*).

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "common.h"
#include "egress_kernel.h"

#ifndef RCFM_PACK_NT
#define RCFM_PACK_NT 0   // plain stores of the packed rows: non-temporal ones measured 13 % (int16) and 27 % (float32) slower
#endif                   // with every channel open, 4 % faster with a tenth open (docs/EXPERIMENTS.md, "pack stores")

namespace rcfm {

namespace {

constexpr int kMaxChannels = 65535;
constexpr bool kPackNT = RCFM_PACK_NT != 0;

// The slot table, library-owned: [65 535] int32, one per stream that has ever packed.  Calls on one stream are ordered, so
// a table has one scan and its readers in flight at a time; calls on different streams never share one.  Plain hipMalloc on
// a stream's first call, kept for the life of the process (256 KiB each), like the other function-static scratch.
int32_t* slot_table(hipStream_t stream) {
    static std::mutex mu;
    static std::map<hipStream_t, int32_t*> tables;
    std::lock_guard<std::mutex> lock(mu);
    auto it = tables.find(stream);
    if (it != tables.end()) return it->second;
    void* p = nullptr;
    RC_HIP(hipMalloc(&p, sizeof(int32_t) * (size_t)kMaxChannels));
    tables[stream] = static_cast<int32_t*>(p);
    return static_cast<int32_t*>(p);
}

template <int FORMAT>
void launch_pack(const float* audio, const int32_t* slot, int count, size_t row, float gain, void* packed, hipStream_t stream) {
    const size_t per_vec = FORMAT == RCFM_PCM_S16 ? 8 : 4;
    const bool vec = row % per_vec == 0 && (uintptr_t)audio % 16 == 0 && (uintptr_t)packed % 16 == 0;
    const size_t segs = (row + kPackSegment - 1) / kPackSegment;
    // fewer than 2^24 workgroups in all (2^32 threads); longer rows take further sweeps of the same grid
    const size_t max_y = std::max<size_t>(((size_t)1 << 24) / (size_t)count - 1, 1);
    const dim3 grid((unsigned)count, (unsigned)std::min({segs, max_y, (size_t)65535}), 1);
    if (vec)
        hipLaunchKernelGGL((k_audio_pack<FORMAT, true, kPackNT>), grid, dim3(kPackThreads), 0, stream, audio, slot, row, gain, packed);
    else
        hipLaunchKernelGGL((k_audio_pack<FORMAT, false, kPackNT>), grid, dim3(kPackThreads), 0, stream, audio, slot, row, gain, packed);
    RC_HIP(hipGetLastError());
}

}  // namespace

}  // namespace rcfm

using namespace rcfm;

// Overlapped device -> host egress (rcfm_drain_*): `depth` slots, a header stream and a payload stream.
struct rcfm_drain_s {
    size_t row_bytes = 0, head_bytes = 0, head_room = 0;   // head_room: the header's share of the host mirror, a multiple of 64
    int max_rows = 0, depth = 0;
    struct Slot {
        void* packed = nullptr;        // device [max_rows][row_bytes]
        int32_t* head = nullptr;       // device: n_open, then index [max_rows]
        char* host = nullptr;          // page-locked: the header, then at head_room the rows
        hipEvent_t packed_ready = nullptr, head_ready = nullptr;
    };
    std::vector<Slot> slot;
    hipStream_t head_stream = nullptr, payload_stream = nullptr;
    uint64_t head = 0, tail = 0;       // submitted / released buffers
    bool acquired = false;             // the oldest submitted slot's payload has landed and its pointers are out
    ~rcfm_drain_s() {
        if (head_stream) (void)hipStreamSynchronize(head_stream);
        if (payload_stream) (void)hipStreamSynchronize(payload_stream);
        for (auto& s : slot) {
            if (s.packed_ready) (void)hipEventDestroy(s.packed_ready);
            if (s.head_ready) (void)hipEventDestroy(s.head_ready);
            if (s.packed) (void)hipFree(s.packed);
            if (s.head) (void)hipFree(s.head);
            if (s.host) (void)hipHostFree(s.host);
        }
        if (head_stream) (void)hipStreamDestroy(head_stream);
        if (payload_stream) (void)hipStreamDestroy(payload_stream);
    }
};

extern "C" {

int rcfm_audio_pack(const void* audio, const void* open, int count, size_t row, int format, float gain, void* packed, void* index,
                    void* n_open, void* stream) {
    return guarded([&] {
        RC_REQUIRE(audio && packed, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(count >= 1 && count <= kMaxChannels, RCFM_ERR_ARG, "count outside 1 .. 65535");
        RC_REQUIRE(row >= 1 && row <= (SIZE_MAX >> 3) / (size_t)kMaxChannels, RCFM_ERR_ARG, "bad row length");
        RC_REQUIRE(format == RCFM_PCM_F32 || format == RCFM_PCM_S16, RCFM_ERR_ARG, "unknown PCM format (RCFM_PCM_F32, RCFM_PCM_S16)");
        if (format == RCFM_PCM_S16)
            RC_REQUIRE(std::isfinite(gain) && gain > 0.0f && gain <= 16777216.0f, RCFM_ERR_ARG, "gain must be finite and in (0, 2^24]");
        const uintptr_t a0 = (uintptr_t)audio, a1 = a0 + (size_t)count * row * sizeof(float);
        const uintptr_t p0 = (uintptr_t)packed, p1 = p0 + (size_t)count * row * (format == RCFM_PCM_S16 ? 2 : 4);
        RC_REQUIRE(a1 <= p0 || p1 <= a0, RCFM_ERR_ARG, "audio and packed overlap");
        RC_REQUIRE(a0 % 4 == 0 && p0 % (format == RCFM_PCM_S16 ? 2 : 4) == 0, RCFM_ERR_ARG,
                   "misaligned buffer: audio is aligned for a float, packed for one sample of the format");
        hipStream_t s = as_stream(stream);
        int32_t* slot = slot_table(s);
        hipLaunchKernelGGL(k_slot_scan, dim3(1), dim3(kScanThreads), 0, s, static_cast<const uint8_t*>(open), count, slot,
                           static_cast<int32_t*>(index), static_cast<int32_t*>(n_open));
        RC_HIP(hipGetLastError());
        if (format == RCFM_PCM_S16)
            launch_pack<RCFM_PCM_S16>(static_cast<const float*>(audio), slot, count, row, gain, packed, s);
        else
            launch_pack<RCFM_PCM_F32>(static_cast<const float*>(audio), slot, count, row, gain, packed, s);
    });
}

// ---- host egress -----------------------------------------------------------------

int rcfm_drain_create(size_t row_bytes, int max_rows, int depth, rcfm_drain_t* out) {
    return guarded([&] {
        RC_REQUIRE(out != nullptr && row_bytes > 0 && max_rows >= 1 && max_rows <= kMaxChannels && depth >= 1 && depth <= 64 &&
                       row_bytes <= (SIZE_MAX >> 2) / (size_t)kMaxChannels,
                   RCFM_ERR_ARG, "bad drain geometry");
        auto d = std::make_unique<rcfm_drain_s>();
        d->row_bytes = row_bytes;
        d->max_rows = max_rows;
        d->depth = depth;
        d->head_bytes = sizeof(int32_t) * ((size_t)max_rows + 1);
        d->head_room = (d->head_bytes + 63) / 64 * 64;
        RC_HIP(hipStreamCreateWithFlags(&d->head_stream, hipStreamNonBlocking));
        RC_HIP(hipStreamCreateWithFlags(&d->payload_stream, hipStreamNonBlocking));
        d->slot.resize((size_t)depth);
        for (auto& s : d->slot) {
            RC_HIP(hipMalloc(&s.packed, row_bytes * (size_t)max_rows));
            void* h = nullptr;
            RC_HIP(hipMalloc(&h, d->head_bytes));
            s.head = static_cast<int32_t*>(h);
            void* m = nullptr;
            RC_HIP(hipHostMalloc(&m, d->head_room + row_bytes * (size_t)max_rows, hipHostMallocDefault));
            s.host = static_cast<char*>(m);
            std::memset(s.host, 0, d->head_room);
            RC_HIP(hipEventCreateWithFlags(&s.packed_ready, hipEventDisableTiming));
            RC_HIP(hipEventCreateWithFlags(&s.head_ready, hipEventDisableTiming));
        }
        *out = d.release();
    });
}

int rcfm_drain_begin(rcfm_drain_t d, void** packed_dev, void** index_dev, void** n_open_dev) {
    return guarded([&] {
        RC_REQUIRE(d && packed_dev && index_dev && n_open_dev, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(d->head - d->tail < (uint64_t)d->depth, RCFM_ERR_STATE,
                   "every drain slot is in flight: acquire and release one before packing another buffer");
        const auto& s = d->slot[(size_t)(d->head % (uint64_t)d->depth)];
        *packed_dev = s.packed;
        *n_open_dev = s.head;
        *index_dev = s.head + 1;
    });
}

int rcfm_drain_submit(rcfm_drain_t d, void* stream) {
    return guarded([&] {
        RC_REQUIRE(d, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(d->head - d->tail < (uint64_t)d->depth, RCFM_ERR_STATE,
                   "every drain slot is in flight: acquire and release one before submitting another buffer");
        auto& s = d->slot[(size_t)(d->head % (uint64_t)d->depth)];
        RC_HIP(hipEventRecord(s.packed_ready, as_stream(stream)));        // the pack of this slot is queued on `stream`
        RC_HIP(hipStreamWaitEvent(d->head_stream, s.packed_ready, 0));
        RC_HIP(hipMemcpyAsync(s.host, s.head, d->head_bytes, hipMemcpyDeviceToHost, d->head_stream));
        RC_HIP(hipEventRecord(s.head_ready, d->head_stream));
        d->head += 1;
    });
}

int rcfm_drain_acquire(rcfm_drain_t d, int* n_open, const int32_t** index_host, const void** rows_host) {
    return guarded([&] {
        RC_REQUIRE(d && n_open && index_host && rows_host, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(d->tail < d->head, RCFM_ERR_STATE, "rcfm_drain_acquire without a submitted buffer");
        auto& s = d->slot[(size_t)(d->tail % (uint64_t)d->depth)];
        const int32_t* head = reinterpret_cast<const int32_t*>(s.host);
        if (!d->acquired) {
            RC_HIP(hipEventSynchronize(s.head_ready));                     // this slot's header only
            const int n = head[0];
            RC_REQUIRE(n >= 0 && n <= d->max_rows, RCFM_ERR_RUNTIME, "the drained header's n_open is outside 0 .. max_rows");
            if (n > 0) {
                // the header has landed, so the pack it waited for is complete: the payload stream needs no event
                RC_HIP(hipMemcpyAsync(s.host + d->head_room, s.packed, (size_t)n * d->row_bytes, hipMemcpyDeviceToHost,
                                      d->payload_stream));
                RC_HIP(hipStreamSynchronize(d->payload_stream));
            }
            d->acquired = true;
        }
        *n_open = head[0];
        *index_host = head + 1;
        *rows_host = s.host + d->head_room;
    });
}

int rcfm_drain_release(rcfm_drain_t d) {
    return guarded([&] {
        RC_REQUIRE(d, RCFM_ERR_ARG, "NULL argument");
        RC_REQUIRE(d->acquired, RCFM_ERR_STATE, "rcfm_drain_release without an acquired buffer");
        d->acquired = false;
        d->tail += 1;
    });
}

int rcfm_drain_destroy(rcfm_drain_t d) {
    return guarded([&] { delete d; });
}

}  // extern "C"
