// The device stage of the PNG decode (csrc/madtp_png.h): zlib streams -> filtered scanlines (png_inflate_kernel), filtered
// scanlines -> packed RGB [h, w, 3] (png_unfilter_kernel), one workgroup of one wave per image in both.  Everything the lanes do is
// in png_device.h, which the host emulation (madtp_png_inflate_host, madtp_png_unfilter_host) runs as well; this file checks the
// table rows and launches.
//
// Visibility.  A workgroup is ONE wave, and everything its lanes hand to each other goes through LDS with a barrier between the
// write and the read (sync_lanes): the inflate window, the Huffman tables, the partial checksums, the unfilter tile.  The match
// copy never reads global memory: the filtered bytes leave for `raw` in halves of the window and are not read back.  The one thing
// read back from global memory is the unfilter kernel's carry, 16 bytes per row that the SAME lane wrote - program order of one
// thread, no fence needed.  No workgroup waits for another, there are no atomics, and every loop is bounded by the stream's bits or
// the image's bytes: identical calls give identical bits.
#include "common.h"

#include "png_device.h"

namespace {

using namespace madtp_png;

__device__ __forceinline__ bool row_format(const int64_t* t, Format& f) {
    const int64_t w = t[MADTP_PNG_F_W], h = t[MADTP_PNG_F_H], depth = t[MADTP_PNG_F_DEPTH], color = t[MADTP_PNG_F_COLOR];
    if (w < 1 || w > MADTP_PNG_MAX_SIDE || h < 1 || h > MADTP_PNG_MAX_SIDE || depth < 1 || depth > 16 || color < 0 || color > 6) return false;
    return make_format(f, w, h, (int)depth, (int)color) == 0 && f.raw_bytes == t[MADTP_PNG_F_RAW_BYTES];
}

__global__ __launch_bounds__(kLanes) void png_inflate_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ table,
                                                             uint8_t* __restrict__ raw, int32_t* __restrict__ status) {
    __shared__ InflateShared sh;
    const int64_t* t = table + (size_t)blockIdx.x * MADTP_PNG_FIELDS;
    int32_t* st = status + (size_t)blockIdx.x * MADTP_PNG_STATUS_FIELDS;
    Format f;
    const int64_t stream_at = t[MADTP_PNG_F_STREAM], stream_bytes = t[MADTP_PNG_F_STREAM_BYTES], raw_at = t[MADTP_PNG_F_RAW];
    if (!row_format(t, f) || stream_at < 0 || stream_bytes < 0 || stream_bytes > 0x7fffffff || raw_at < 0 || (raw_at & 3)) {  // (uniform)
        if (threadIdx.x == 0) st[MADTP_PNG_S_CODE] = MADTP_E_BADARG, st[MADTP_PNG_S_BLOCKS] = 0, st[MADTP_PNG_S_BYTES] = 0, st[MADTP_PNG_S_ADLER] = 0;
        return;
    }
    inflate_image(sh, bytes + stream_at, stream_bytes, raw + raw_at, f.raw_bytes, f.rowbytes, st);
}

__global__ __launch_bounds__(kLanes) void png_unfilter_kernel(const uint8_t* __restrict__ raw, const int64_t* __restrict__ table,
                                                              const uint8_t* __restrict__ palette, uint8_t* __restrict__ out) {
    __shared__ UnfilterShared sh;
    const int64_t* t = table + (size_t)blockIdx.x * MADTP_PNG_FIELDS;
    Format f;
    const int64_t raw_at = t[MADTP_PNG_F_RAW], out_at = t[MADTP_PNG_F_OUT], palette_at = t[MADTP_PNG_F_PALETTE], carry_at = t[MADTP_PNG_F_CARRY];
    if (!row_format(t, f) || raw_at < 0 || out_at < 0 || palette_at < 0 || carry_at < 0 || (carry_at & 15)) return;  // (uniform)
    unfilter_image(sh, f, raw + raw_at, palette + palette_at, out + out_at, out + carry_at);
}

}  // namespace

extern "C" int madtp_png_abi_version(void) { return MADTP_PNG_ABI_VERSION; }

extern "C" const char* madtp_png_strerror(int code) {
    const char* s = madtp_png::strerror_png(code);
    return s ? s : madtp_strerror(code);
}

extern "C" int madtp_png_prepare(const void* data, int64_t size, int32_t* info, void* palette, void* stream, int64_t stream_capacity) {
    if (!data || size < 0 || !info || !palette || stream_capacity < 0) return MADTP_E_BADARG;
    return madtp_png::prepare((const uint8_t*)data, size, info, (uint8_t*)palette, (uint8_t*)stream, stream_capacity);
}

extern "C" int64_t madtp_png_rowbytes(int w, int depth, int color) {
    Format f;
    return madtp_png::make_format(f, w, 1, depth, color) ? 0 : f.rowbytes;
}

extern "C" int64_t madtp_png_raw_bytes(int w, int h, int depth, int color) {
    Format f;
    return madtp_png::make_format(f, w, h, depth, color) ? 0 : f.raw_bytes;
}

extern "C" int64_t madtp_png_carry_bytes(int h) { return h < 1 || h > MADTP_PNG_MAX_SIDE ? 0 : 16 * (int64_t)h; }

extern "C" int madtp_png_inflate_host(const void* stream, int64_t stream_bytes, void* raw, int64_t raw_bytes, int rowbytes, int32_t* status) {
    return madtp_png::inflate_host((const uint8_t*)stream, stream_bytes, (uint8_t*)raw, raw_bytes, rowbytes, status);
}

extern "C" int madtp_png_unfilter_host(const void* raw, int w, int h, int depth, int color, const void* palette, void* out) {
    if (h < 1 || h > MADTP_PNG_MAX_SIDE) return MADTP_E_BADARG;
    uint8_t carry[16 * MADTP_PNG_MAX_SIDE];
    return madtp_png::unfilter_host((const uint8_t*)raw, w, h, depth, color, (const uint8_t*)palette, (uint8_t*)out, carry);
}

extern "C" int madtp_png_inflate_batch(const void* bytes, const int64_t* table, void* raw, int32_t* status, int B, void* stream) {
    if (!bytes || !table || !raw || !status || B < 1) return MADTP_E_BADARG;
    hipLaunchKernelGGL(png_inflate_kernel, dim3(B), dim3(kLanes), 0, (hipStream_t)stream, (const uint8_t*)bytes, table, (uint8_t*)raw, status);
    MADTP_LAUNCH_CHECK();
    return 0;
}

extern "C" int madtp_png_unfilter_batch(const void* raw, const int64_t* table, const void* palette, void* out, int B, void* stream) {
    if (!raw || !table || !palette || !out || B < 1) return MADTP_E_BADARG;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3(B), dim3(kLanes), 0, (hipStream_t)stream, (const uint8_t*)raw, table,
                       (const uint8_t*)palette, (uint8_t*)out);
    MADTP_LAUNCH_CHECK();
    return 0;
}
