// orbx_color.hip -- BGR / RGB / BGRA / RGBA frames to the grey plane the extractor works on (level 0 of the pyramid).
//
// Arithmetic: OpenCV 3.1.0's portable 8-bit RGB2Gray (modules/imgproc/src/color.cpp: R2Y = 4899, G2Y = 9617, B2Y = 1868,
// yuv_shift = 14), grey = (4899 R + 9617 G + 1868 B + 8192) >> 14, alpha ignored.  The coefficients sum to 2^14, so the result is
// at most 255 and needs no saturation.  Integers only: nothing here depends on the floating-point mode.
//
// The kernel is bandwidth-bound (3 or 4 bytes read, 1 written per pixel).  One thread makes four neighbouring pixels of one row and
// stores them as ONE dword into the handle's grey block, whose rows start on 64-byte boundaries and whose pitch covers the width
// rounded up to 4 (the bytes of a last, partial quad beyond the width are written as 0; nothing reads them).  The source is the
// caller's: its row stride is arbitrary, so the alignment of a row's first byte changes from row to row.  A quad inside a row
// whose base is 4-aligned is read with three dword loads (BGR: 12 bytes) or one 16-byte load (BGRA, 16-aligned; four dword loads
// when only 4-aligned); every other quad -- a misaligned row, or the last quad of a width that is no multiple of 4 -- is read
// byte by byte.  No path reads a byte at or beyond row + width * channels: a wide load is issued only for a quad that lies wholly
// inside the row, and it covers exactly that quad's bytes.
//
// Indexing: a row offset y * stride and a pixel offset are 32-bit inside a frame (the callers check frame < 2 GiB, stride < 8 MiB);
// the frame offset is 64-bit.
#include "orbx_internal.h"

#define COLOR_BX 32           // quads across a workgroup: a wave covers 2 rows x 128 pixels (384 / 512 contiguous source bytes per row)
#define COLOR_BY 8

template <bool RGB> __device__ __forceinline__ uint32_t to_grey(uint32_t c0, uint32_t c1, uint32_t c2)
{
    const uint32_t r = RGB ? c0 : c2, b = RGB ? c2 : c0;
    return (4899u * r + 9617u * c1 + 1868u * b + 8192u) >> 14;
}

template <int CN, bool RGB> __global__ __launch_bounds__(COLOR_BX * COLOR_BY)
void k_color_to_grey(const uint8_t *__restrict__ src, int src_stride, long long src_frame,
                     uint8_t *__restrict__ dst, int dst_stride, long long dst_frame, int W, int H)
{
    const int x0 = (blockIdx.x * COLOR_BX + threadIdx.x) * 4;
    const int y = blockIdx.y * COLOR_BY + threadIdx.y;
    if (x0 >= W || y >= H) return;
    const uint8_t *row = src + (long long)blockIdx.z * src_frame + (long long)y * src_stride;
    const uint8_t *p = row + x0 * CN;
    uint32_t out = 0;
    if (x0 + 4 <= W && ((uintptr_t)row & 3) == 0) {          // the whole quad lies inside the row and p is 4-aligned (x0 * CN is a multiple of 4)
        if (CN == 3) {
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];   // bytes 0..11 = four pixels
            out = to_grey<RGB>(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u)
                | to_grey<RGB>(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u) << 8
                | to_grey<RGB>((w1 >> 16) & 255u, w1 >> 24, w2 & 255u) << 16
                | to_grey<RGB>((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24) << 24;
        } else {
            uint4 v;
            if (((uintptr_t)row & 15) == 0) v = *reinterpret_cast<const uint4 *>(p);
            else { const uint32_t *q = reinterpret_cast<const uint32_t *>(p); v = make_uint4(q[0], q[1], q[2], q[3]); }
            out = to_grey<RGB>(v.x & 255u, (v.x >> 8) & 255u, (v.x >> 16) & 255u)
                | to_grey<RGB>(v.y & 255u, (v.y >> 8) & 255u, (v.y >> 16) & 255u) << 8
                | to_grey<RGB>(v.z & 255u, (v.z >> 8) & 255u, (v.z >> 16) & 255u) << 16
                | to_grey<RGB>(v.w & 255u, (v.w >> 8) & 255u, (v.w >> 16) & 255u) << 24;
        }
    } else {
        const int n = min(4, W - x0);                         // pixels of this quad inside the row
        for (int i = 0; i < n; i++) out |= to_grey<RGB>(p[i * CN], p[i * CN + 1], p[i * CN + 2]) << (8 * i);
    }
    *reinterpret_cast<uint32_t *>(dst + (long long)blockIdx.z * dst_frame + (long long)y * dst_stride + x0) = out;
}

// nframes frames of W x H pixels in `format` (ORBX_FMT_BGR8 .. ORBX_FMT_RGBA8) -> grey; dst rows 4-aligned, dst_stride >= W rounded up to 4
void orbx_launch_color(const uint8_t *src, int src_stride, long long src_frame, uint8_t *dst, int dst_stride, long long dst_frame,
                       int W, int H, int nframes, int format, hipStream_t s)
{
    const dim3 block(COLOR_BX, COLOR_BY);
    for (int f0 = 0; f0 < nframes; f0 += 65535) {             // grid.z is 16 bits wide
        const int nf = nframes - f0 < 65535 ? nframes - f0 : 65535;
        const dim3 grid((W + 4 * COLOR_BX - 1) / (4 * COLOR_BX), (H + COLOR_BY - 1) / COLOR_BY, nf);
        const uint8_t *sp = src + (long long)f0 * src_frame;
        uint8_t *dp = dst + (long long)f0 * dst_frame;
        switch (format) {
        case ORBX_FMT_BGR8:  k_color_to_grey<3, false><<<grid, block, 0, s>>>(sp, src_stride, src_frame, dp, dst_stride, dst_frame, W, H); break;
        case ORBX_FMT_RGB8:  k_color_to_grey<3, true><<<grid, block, 0, s>>>(sp, src_stride, src_frame, dp, dst_stride, dst_frame, W, H); break;
        case ORBX_FMT_BGRA8: k_color_to_grey<4, false><<<grid, block, 0, s>>>(sp, src_stride, src_frame, dp, dst_stride, dst_frame, W, H); break;
        case ORBX_FMT_RGBA8: k_color_to_grey<4, true><<<grid, block, 0, s>>>(sp, src_stride, src_frame, dp, dst_stride, dst_frame, W, H); break;
        default: break;
        }
    }
}
