// The Huffman entropy stage of the JPEG decode on the device (include/madtp_jhuff.h): one workgroup of MADTP_JHUFF_LANES lanes per
// image, one thread per subsequence of the scan.  Everything a lane does is in jpeg_huff_device.h, which the host emulation
// (madtp_jhuff_decode_host) runs as well; this file holds the order of the phases with the barriers between them, and it must stay
// line for line the order of decode_image_host there.
//
// The Huffman tables of the image (8.5 KB) and the lanes' states live in LDS; the file's bytes are read from global memory a byte at
// a time into a 64-bit register buffer (they are read once per pass, by neighbouring lanes, and stay in the cache).  Lanes of a
// wave diverge inside lane_run - symbols differ - and meet again at the barrier behind every phase.  No workgroup waits for another;
// the one atomic is an integer minimum in LDS, whose result does not depend on the order of arrival.
#include "common.h"

#include "jpeg_huff_device.h"

namespace {

using namespace madtp_jhuff;

__device__ const uint8_t kZigzagDevice[64] = {
    0,  8,  1,  2,  9,  16, 24, 17, 10, 3,  4,  11, 18, 25, 32, 40, 33, 26, 19, 12, 5,  6,  13, 20, 27, 34, 41, 48, 56, 49, 42, 35,
    28, 21, 14, 7,  15, 22, 29, 36, 43, 50, 57, 58, 51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63};

__device__ __forceinline__ void zero_coefficients(int16_t* coef, int64_t blocks) {
    uint32_t* c = (uint32_t*)coef;
    for (int64_t i = threadIdx.x; i < 32 * blocks; i += kLanes) c[i] = 0u;
}

__global__ __launch_bounds__(kLanes) void jhuff_decode_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ table,
                                                              uint8_t* __restrict__ coef_base, int32_t* __restrict__ status,
                                                              int subseq_bytes) {
    __shared__ Shared sh;
    __shared__ uint8_t zz[64];
    const int64_t* t = table + (size_t)blockIdx.x * MADTP_JHUFF_FIELDS;
    int32_t* st = status + (size_t)blockIdx.x * MADTP_JHUFF_STATUS_FIELDS;
    const int j = threadIdx.x;
    const int64_t file_at = t[MADTP_JHUFF_F_FILE], record_at = t[MADTP_JHUFF_F_RECORD], coef_at = t[MADTP_JHUFF_F_COEF];
    Image im;
    const bool ok = file_at >= 0 && record_at >= 0 && (record_at & 3) == 0 && coef_at >= 0 && (coef_at & 3) == 0 &&
                    t[MADTP_JHUFF_F_COMPONENTS] >= 0 && t[MADTP_JHUFF_F_COMPONENTS] <= 3 && t[MADTP_JHUFF_F_HS] >= 0 &&
                    t[MADTP_JHUFF_F_HS] <= 4 && t[MADTP_JHUFF_F_VS] >= 0 && t[MADTP_JHUFF_F_VS] <= 4 && t[MADTP_JHUFF_F_BLOCKS_X] >= 0 &&
                    t[MADTP_JHUFF_F_BLOCKS_X] <= 65535 && t[MADTP_JHUFF_F_BLOCKS_Y] >= 0 && t[MADTP_JHUFF_F_BLOCKS_Y] <= 65535 &&
                    t[MADTP_JHUFF_F_RESTART] >= 0 && t[MADTP_JHUFF_F_RESTART] <= 65535 &&
                    make_image(im, bytes + file_at, t[MADTP_JHUFF_F_SIZE], t[MADTP_JHUFF_F_SCAN], (int)t[MADTP_JHUFF_F_COMPONENTS],
                               (int)t[MADTP_JHUFF_F_HS], (int)t[MADTP_JHUFF_F_VS], (int)t[MADTP_JHUFF_F_BLOCKS_X],
                               (int)t[MADTP_JHUFF_F_BLOCKS_Y], (int)t[MADTP_JHUFF_F_RESTART], subseq_bytes);
    if (!ok) {  // (uniform: before any barrier)
        if (j == 0) st[MADTP_JHUFF_S_CODE] = MADTP_E_BADARG, st[MADTP_JHUFF_S_PASSES] = 0, st[MADTP_JHUFF_S_SUBSEQS] = 0, st[MADTP_JHUFF_S_SERIAL] = 0;
        return;
    }
    im.zz = zz;
    int16_t* coef = (int16_t*)(coef_base + coef_at);
    {
        const uint32_t* src = (const uint32_t*)(bytes + record_at);
        uint32_t* dst = (uint32_t*)sh.tab;
        for (int i = j; i < MADTP_JHUFF_RECORD_BYTES / 4; i += kLanes) dst[i] = src[i];
        if (j < 64) zz[j] = kZigzagDevice[j];
    }
    zero_coefficients(coef, im.blocks);
    if (j == 0) {
        sh.again[0] = sh.again[1] = 0;
        sh.carry_pos = (uint32_t)(im.scan * 8), sh.carry_bk = 0, sh.carry_blocks = 0;
    }
    __syncthreads();

    int code = MADTP_JPEG_E_TRUNCATED, passes = 0, serial = 0;
    bool over = false;
    for (int64_t g0 = 0; g0 < im.lanes && !over; g0 += kLanes) {
        const int lanes = (int)(im.lanes - g0 < kLanes ? im.lanes - g0 : kLanes);
        if (j < lanes) phase_first(im, sh, g0, j);
        ++passes;
        __syncthreads();
        for (int pass = 2; pass <= lanes; ++pass) {
            const int f = pass & 1;
            if (j < lanes && phase_compare(sh, j)) sh.again[f] = 1;
            if (j == 0) sh.again[f ^ 1] = 0;
            __syncthreads();
            if (!sh.again[f]) break;  // (uniform: every lane reads the same word behind the barrier)
            if (j < lanes) phase_again(im, sh, g0, j);
            ++passes;
            __syncthreads();
        }
        int to = 0;
        if (j < lanes) phase_sum(sh, j, 0, to);
        if (j == 0) sh.first_bad = lanes, sh.again[0] = sh.again[1] = 0;  // (a lane still at the `break` above reads 0 either way)
        __syncthreads();
        for (int d = 1; d < lanes; d <<= 1) {
            to ^= 1;
            if (j < lanes) phase_sum(sh, j, d, to);
            __syncthreads();
        }
        if (j < lanes) phase_write(im, sh, g0, j, to, coef);
        __syncthreads();
        if (j < lanes && phase_chain(sh, j, lanes)) atomicMin(&sh.first_bad, j);
        __syncthreads();
        const int first_bad = sh.first_bad;
        if (first_bad < lanes) {
            over = true;
            if (sh.u.l.xbk[first_bad] == kTerminal) {
                code = sh.u.l.xcode[first_bad];
            } else {  // the lanes' guesses and the exact rules parted: one lane, from the beginning
                serial = 1;
                zero_coefficients(coef, im.blocks);
                __syncthreads();
                if (j == 0) sh.again[0] = lane_run(im, sh.tab, (uint32_t)(im.scan * 8), 0, 0, kNoBoundary, coef).code;
                __syncthreads();
                code = sh.again[0];
            }
        } else {
            if (j == 0) {
                sh.carry_pos = sh.u.l.xpos[lanes - 1], sh.carry_bk = sh.u.l.xbk[lanes - 1];
                sh.carry_blocks += sh.u.l.sum[to][lanes - 1];
            }
        }
        __syncthreads();
    }
    if (code == 0) {  // (uniform) the lane arrays are read no more: the sums take their place
        phase_dc_local(im, sh, j, coef);
        __syncthreads();
        int to = 0;
        for (int d = 1; d < kLanes; d <<= 1) {
            to ^= 1;
            phase_dc_sum(sh, j, d, to);
            __syncthreads();
        }
        phase_dc_write(im, sh, j, to, coef);
    }
    if (j == 0) st[MADTP_JHUFF_S_CODE] = code, st[MADTP_JHUFF_S_PASSES] = passes, st[MADTP_JHUFF_S_SUBSEQS] = im.lanes, st[MADTP_JHUFF_S_SERIAL] = serial;
}

}  // namespace

extern "C" int madtp_jhuff_abi_version(void) { return MADTP_JHUFF_ABI_VERSION; }

extern "C" int madtp_jhuff_subseq_bytes(int64_t scan_bytes) { return madtp_jhuff::default_subseq(scan_bytes); }

extern "C" int madtp_jhuff_prepare(const void* data, int64_t size, int32_t* info, void* qtables, void* tables, int64_t* scan_begin) {
    if (((uintptr_t)tables & 3u) != 0) return MADTP_E_BADARG;
    madtp_jpeg::Header h;
    return madtp_jhuff::prepare((const uint8_t*)data, size, info, (uint16_t*)qtables, (madtp_jhuff::Table*)tables, scan_begin, h);
}

extern "C" int madtp_jhuff_decode_host(const void* data, int64_t size, int subseq_bytes, void* coef, int64_t coef_capacity, int32_t* status) {
    madtp_jpeg::Header h;
    madtp_jhuff::Shared sh;
    return madtp_jhuff::decode_host((const uint8_t*)data, size, subseq_bytes, (int16_t*)coef, coef_capacity, status, h, sh);
}

extern "C" int madtp_jhuff_decode_batch(const void* bytes, const int64_t* table, void* coef, int32_t* status, int B, int subseq_bytes,
                                        void* stream) {
    if (!bytes || !table || !coef || !status || B < 1 || subseq_bytes < 0 || (subseq_bytes & 3)) return MADTP_E_BADARG;
    hipLaunchKernelGGL(jhuff_decode_kernel, dim3(B), dim3(kLanes), 0, (hipStream_t)stream, (const uint8_t*)bytes, table, (uint8_t*)coef,
                       status, subseq_bytes);
    MADTP_LAUNCH_CHECK();
    return 0;
}
