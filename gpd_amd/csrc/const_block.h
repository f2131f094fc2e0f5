// The device-wide constant blocks (hands.hip c_hand, images.hip c_img) and the one way they are loaded.
//
// A __constant__ block is ONE per device, shared by every context of the process on that device.  Under the block's
// lock: a context whose bytes (geometry, tables) differ from the loaded ones waits for the device — kernels of another
// context, on another stream, may still be reading the block — and loads its own; the lock is handed back to the
// caller, who keeps it until its kernels that read the block are enqueued.  Same-stream order covers the context's own
// earlier kernels.
#pragma once
#include <cstring>
#include <mutex>
#include <vector>

#include "gpd_internal.h"

namespace gpd {

struct ConstBlock {
  std::mutex mutex;
  std::vector<unsigned char> loaded[64];  // per device: the bytes the block holds

  // Takes the lock and makes `bytes` of `want` the contents of `symbol` on the current device.
  template <class SYMBOL>
  int load(const SYMBOL &symbol, const void *want, size_t bytes, hipStream_t stream, std::unique_lock<std::mutex> &lock) {
    lock = std::unique_lock<std::mutex>(mutex);
    int dev = 0;
    HIP_RET(hipGetDevice(&dev));
    std::vector<unsigned char> &have = loaded[dev & 63];
    if (have.size() == bytes && std::memcmp(have.data(), want, bytes) == 0) return GPD_OK;
    if (!have.empty()) HIP_RET(hipDeviceSynchronize());
    HIP_RET(hipMemcpyToSymbolAsync(HIP_SYMBOL(symbol), want, bytes, 0, hipMemcpyHostToDevice, stream));
    // the block counts as loaded only once the copy has landed: a context with the same values skips
    // the copy and launches on ITS stream, which is not ordered after this one
    HIP_RET(hipStreamSynchronize(stream));
    const unsigned char *b = static_cast<const unsigned char *>(want);
    have.assign(b, b + bytes);
    return GPD_OK;
  }
};

}  // namespace gpd
