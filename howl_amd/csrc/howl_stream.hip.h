// What the entry points of the one-launch window kernels (res8_stream.hip, las_stream.hip, gru_stream.hip) share on the host.  The
// softmax that ends the three kernels is not here: as a function it changes one instruction in each (profiles/stream_refactor_isa.txt).
#pragma once
#include "howl_common.hip.h"

namespace {

// 8-byte sample loads need every window's first sample 8-byte aligned; anything else takes the per-sample path
inline int stream_pcm_aligned(const float* pcm, long ld, int N) {
    return ((N == 1 || (ld & 1) == 0) && (reinterpret_cast<uintptr_t>(pcm) & 7) == 0) ? 1 : 0;
}

// every pointer of a record that consists of `const float*` fields only is non-null
template <class Record>
inline bool stream_record_complete(const Record* r) {
    const float* const* fields = reinterpret_cast<const float* const*>(r);
    bool all = true;
    for (size_t i = 0; i < sizeof(Record) / sizeof(const float*); ++i) all = all && fields[i] != nullptr;
    return all;
}

}  // namespace

// The launch geometry of entry point `name` (a string literal): 1..max_windows windows of L samples, ld >= 0 samples apart, every
// sample offset inside 32 bits.  Returns HOWL_E_ARG from the entry point with the error text set.
#define HOWL_STREAM_REQUIRE_GEOMETRY(name, N, max_windows, ld, L)                                                              \
    do {                                                                                                                        \
        HOWL_REQUIRE((N) >= 1 && (N) <= (max_windows), name ": N=%d windows unsupported (1..%d)", (N), (max_windows));           \
        HOWL_REQUIRE((ld) >= 0, name ": negative window stride %ld", (ld));                                                      \
        HOWL_REQUIRE((long)((N) - 1) * (ld) + (L) < (1L << 31), name ": the windows span %ld samples (32-bit sample offsets)",   \
                     (long)((N) - 1) * (ld) + (L));                                                                              \
    } while (0)
