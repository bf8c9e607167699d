// cub_calls.h -- the hipCUB scans and sorts of the mesh kernels, and the read-back that ends a count phase.  Two kinds of call:
//   the exact scratch queries, for the layouts that size their scratch by asking hipCUB (they return hipCUB's status: a layout that ignored it
//   would report a workspace with no scratch in it);
//   the checked calls, which ask for the scratch of the call at hand first and refuse one that exceeds what the layout reserved, whether that
//   was an exact query or the bound of ws_plan.h.  `what` is the message nero_last_error() reports; a call refused before it ran appends why.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <stdio.h>
#include "common.h"
#include "../../include/nero_hip.h"

namespace nero_cub {

// scratch bytes of a prefix sum over `items` values of T
template <typename T>
hipError_t scan_temp(int64_t items, size_t* bytes) {
    *bytes = 0;
    return hipcub::DeviceScan::ExclusiveSum((void*)nullptr, *bytes, (const T*)nullptr, (T*)nullptr, (int)items);
}

// scratch bytes of a radix sort of `items` (K key, unsigned value) pairs over the low `bits` bits (the histograms grow with the bits); no
// items, no scratch
template <typename K>
hipError_t sort_pairs_temp(int64_t items, int bits, size_t* bytes) {
    *bytes = 0;
    if (items <= 0) return hipSuccess;
    return hipcub::DeviceRadixSort::SortPairs((void*)nullptr, *bytes, (const K*)nullptr, (K*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr,
                                              (int)items, 0, bits);
}

// a checked call that did not run: `what`, and whether its own size query failed or asks for more than the layout reserved
inline int refuse(const char* what, bool query_failed) {
    static thread_local char msg[256];
    snprintf(msg, sizeof(msg), "%s (%s)", what, query_failed ? "its scratch-size query failed" : "its scratch exceeds what the workspace reserved");
    return nero_fail(NERO_ERR_LAUNCH, msg);
}

// a *_workspace_bytes that refuses its sizes: 0, with the reason on record as it is when a layout's query fails
inline size_t no_workspace(const char* why) {
    nero_fail(NERO_ERR_UNSUPPORTED, why);
    return 0;
}

template <typename In, typename Out>
int exclusive_sum(void* temp, size_t temp_bytes, In in, Out* out, int64_t items, hipStream_t s, const char* what) {
    size_t need = 0;
    const bool query_failed = hipcub::DeviceScan::ExclusiveSum((void*)nullptr, need, in, out, (int)items, s) != hipSuccess;
    if (query_failed || need > temp_bytes) return refuse(what, query_failed);
    if (hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, in, out, (int)items, s) != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, what);
    return NERO_OK;
}

template <typename In, typename Out>
int inclusive_sum(void* temp, size_t temp_bytes, In in, Out* out, int64_t items, hipStream_t s, const char* what) {
    size_t need = 0;
    const bool query_failed = hipcub::DeviceScan::InclusiveSum((void*)nullptr, need, in, out, (int)items, s) != hipSuccess;
    if (query_failed || need > temp_bytes) return refuse(what, query_failed);
    if (hipcub::DeviceScan::InclusiveSum(temp, temp_bytes, in, out, (int)items, s) != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, what);
    return NERO_OK;
}

// stable, ascending, over the low `bits` bits of the keys
template <typename K>
int sort_pairs(void* temp, size_t temp_bytes, const K* kin, K* kout, const unsigned* vin, unsigned* vout, int64_t items, int bits, hipStream_t s,
               const char* what) {
    size_t need = 0;
    const bool query_failed = hipcub::DeviceRadixSort::SortPairs((void*)nullptr, need, kin, kout, vin, vout, (int)items, 0, bits, s) != hipSuccess;
    if (query_failed || need > temp_bytes) return refuse(what, query_failed);
    if (hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, kin, kout, vin, vout, (int)items, 0, bits, s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, what);
    return NERO_OK;
}

// the one synchronisation of a two-phase entry point: the header its count phase left on the device
inline int read_back(void* host, const void* dev, size_t bytes, hipStream_t s, const char* what) {
    if (hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, what);
    return NERO_OK;
}

}  // namespace nero_cub
