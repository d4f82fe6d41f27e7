// conv_wgrad_decode.h — (output pixel, tap) -> source row of the conv weight gradient (comat_conv2d_wgrad).
// ONE copy of the mapping, used by the DMA gather of the pipelined kernel (gemm2.hip), by the general kernel (wgrad.hip) and by
// the stand-alone host program tests/conv_wgrad_decode_check.cpp, which enumerates every (pixel, tap) of the test geometries and
// proves bounds and values on the CPU before the gather ever runs on a device.  Plain C++: no HIP header needed on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define COMAT_HD __host__ __device__
#else
#define COMAT_HD
#endif

struct ConvWgradGeom {
    int B, Hin, Win, Cin;  // X: [B, Hin, Win, Cin] dense channels-last
    int Hout, Wout;        // dY: [B, Hout, Wout, Cout]
    int KW;                // taps per kernel row (KH == KW); tap = kh * KW + kw
    int stride, pad, ups;  // comat_conv2d mode 0: src = dst * stride + k - pad in the `ups`-times nearest-upsampled input
};

constexpr int64_t CONV_WGRAD_ZERO = -1;  // the (pixel, tap) pair contributes nothing: the gather reads the zero page

// Output pixel p = (b * Hout + oy) * Wout + ox (the k-row of the weight-gradient product) and tap -> ELEMENT offset of the Cin
// channels X[b, iy, ix, :] that the forward conv multiplied into dY[p, :] through weight tap (kh, kw), or CONV_WGRAD_ZERO for a
// padding tap and for k-rows p >= B * Hout * Wout (the ragged end of the last k-tile).  A result other than CONV_WGRAD_ZERO lies
// in [0, B * Hin * Win * Cin) on a multiple of Cin, in the image b of the pixel: a tap never crosses into a neighbouring image.
// Requires B * Hout * Wout < 2^31 (the host checks).
COMAT_HD inline int64_t conv_wgrad_src(const ConvWgradGeom& g, int64_t p, int tap) {
    const unsigned hw = (unsigned)g.Hout * (unsigned)g.Wout;
    if (p < 0 || p >= (int64_t)g.B * hw) return CONV_WGRAD_ZERO;
    const unsigned up = (unsigned)p;
    const unsigned b = up / hw, rem = up - b * hw;
    const unsigned oy = rem / (unsigned)g.Wout, ox = rem - oy * (unsigned)g.Wout;
    const int kh = tap / g.KW, kw = tap - kh * g.KW;
    const int y = (int)oy * g.stride + kh - g.pad, x = (int)ox * g.stride + kw - g.pad;  // in the upsampled input
    if (y < 0 || x < 0 || y >= g.Hin * g.ups || x >= g.Win * g.ups) return CONV_WGRAD_ZERO;
    const int iy = g.ups == 2 ? y >> 1 : y, ix = g.ups == 2 ? x >> 1 : x;
    return (((int64_t)b * g.Hin + iy) * g.Win + ix) * g.Cin;
}
