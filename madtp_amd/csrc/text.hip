// Text input on the device (csrc/madtp_text.h): one kernel, one workgroup per text.  Everything the lanes do is in text_device.h,
// which the host emulation (madtp_text_encode_host) runs as well; this file checks the arguments and launches.
//
// Visibility.  Lanes of a workgroup hand data to each other through LDS only, with a barrier between the write and the read
// (sync_lanes).  Global memory is read (the text's bytes inside its extent, the two tables inside their own sizes) or written (the
// text's row and its two status words, every cell by one lane), never read back.  No workgroup waits for another, there are no
// atomics, and every loop is bounded by a launch argument, a table header or the text's bytes: identical calls give identical bits.
#include "common.h"

#include "text_device.h"

namespace {

using namespace madtp_text;

__global__ __launch_bounds__(kLanes) void text_encode_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ chartable, const uint32_t* __restrict__ vocab,
                                                             int64_t* __restrict__ ids_out, int64_t* __restrict__ mask_out,
                                                             int32_t* __restrict__ status, int width, int max_tokens, int flags) {
    __shared__ Shared sh;
    encode_text(sh, bytes, offsets, chartable, vocab, ids_out, mask_out, status, (int)blockIdx.x, width, max_tokens, flags);
}

}  // namespace

extern "C" int madtp_text_abi_version(void) { return MADTP_TEXT_ABI_VERSION; }

extern "C" const char* madtp_text_strerror(int code) {
    const char* s = madtp_text::strerror_text(code);
    return s ? s : madtp_strerror(code);
}

extern "C" int madtp_text_chartable_check(const uint32_t* table, int64_t words) { return madtp_text::chartable_check(table, words); }

extern "C" int64_t madtp_text_vocab_bytes(const void* entries, const int64_t* entry_offsets, int n, int n_special) {
    const int64_t words = madtp_text::vocab_words(entries, entry_offsets, n, n_special);
    return words < 0 ? words : words * 4;
}

extern "C" int madtp_text_vocab_build(const void* entries, const int64_t* entry_offsets, int n, const int32_t* specials, int n_special,
                                      void* out, int64_t out_bytes) {
    return madtp_text::vocab_build(entries, entry_offsets, n, specials, n_special, out, out_bytes);
}

extern "C" int madtp_text_encode_batch(const void* bytes, const int64_t* offsets, const uint32_t* chartable, const uint32_t* vocab,
                                       int64_t* ids_out, int64_t* mask_out, int32_t* status, int B, int width, int max_tokens, int flags,
                                       void* stream) {
    if (int rc = encode_args(bytes, offsets, chartable, vocab, ids_out, mask_out, status, B, width, max_tokens, flags)) return rc;
    hipLaunchKernelGGL(text_encode_kernel, dim3(B), dim3(kLanes), 0, (hipStream_t)stream, (const uint8_t*)bytes, offsets, chartable, vocab,
                       ids_out, mask_out, status, width, max_tokens, flags);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_text_encode_host(const void* bytes, const int64_t* offsets, const uint32_t* chartable, const uint32_t* vocab,
                                      int64_t* ids_out, int64_t* mask_out, int32_t* status, int B, int width, int max_tokens, int flags) {
    return madtp_text::encode_host(bytes, offsets, chartable, vocab, ids_out, mask_out, status, B, width, max_tokens, flags);
}
