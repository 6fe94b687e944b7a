// Host baseline of tools/bench_color.py: the colour-to-grey formula of my-slam_amd/csrc/orbx_color.hip as a plain single-thread loop
// (g++ -O2).  This is NOT OpenCV's cvtColor, whose SIMD paths are faster; it is what the formula costs on one core without them.
#include <stdint.h>
#include <stddef.h>

extern "C" void color_host_loop(const uint8_t *src, uint8_t *dst, size_t npixels, int cn, int rgb)
{
    const int ri = rgb ? 0 : 2, bi = rgb ? 2 : 0;
    for (size_t i = 0; i < npixels; i++) {
        const uint8_t *p = src + i * (size_t)cn;
        dst[i] = (uint8_t)((4899u * p[ri] + 9617u * p[1] + 1868u * p[bi] + 8192u) >> 14);
    }
}
