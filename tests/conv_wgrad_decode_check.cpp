// Stand-alone host check of comat_amd/csrc/conv_wgrad_decode.h (built and run by tests/test_conv_wgrad.py with g++; no GPU).
// For every geometry on the command line (B Hin Win Cin Cout k stride ups, eight integers each) it enumerates every k-row the
// pipelined kernel can issue - every output pixel, and the ragged end of the last 32-row k-tile and one k-tile more - times every
// tap, and checks conv_wgrad_src against the definition of comat_conv2d_wgrad written out independently here:
//   * the result is the zero page or an element offset inside [0, B * Hin * Win * Cin) on a multiple of Cin;
//   * it is the zero page exactly where the definition has a padding tap or no pixel;
//   * otherwise it is the offset of X[b, iy, ix, :] of the pixel's OWN image b, with (iy, ix) the nearest-upsample source of
//     (oy * stride + kh - pad, ox * stride + kw - pad).
// It also counts, per tap, the (pixel, tap) pairs that contribute, against the closed form.  Prints one line per geometry; exit
// status 0 iff everything holds.
#include <cstdio>
#include <cstdlib>

#include "../comat_amd/csrc/conv_wgrad_decode.h"

static long long fails = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            if (fails++ < 20) {           \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
        }                                 \
    } while (0)

// valid output positions o in [0, nout) with 0 <= o * stride + k - pad < nin_up
static long long count_axis(int nout, int stride, int k, int pad, int nin_up) {
    long long n = 0;
    for (int o = 0; o < nout; ++o) {
        const int s = o * stride + k - pad;
        n += s >= 0 && s < nin_up;
    }
    return n;
}

int main(int argc, char** argv) {
    if (argc < 9 || (argc - 1) % 8) {
        std::printf("usage: %s (B Hin Win Cin Cout k stride ups)...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 8 <= argc; a += 8) {
        const int B = std::atoi(argv[a]), Hin = std::atoi(argv[a + 1]), Win = std::atoi(argv[a + 2]), Cin = std::atoi(argv[a + 3]);
        const int k = std::atoi(argv[a + 5]), stride = std::atoi(argv[a + 6]), ups = std::atoi(argv[a + 7]);
        const int pad = k / 2;
        const int Hout = (Hin * ups + 2 * pad - k) / stride + 1, Wout = (Win * ups + 2 * pad - k) / stride + 1;
        const ConvWgradGeom g = {B, Hin, Win, Cin, Hout, Wout, k, stride, pad, ups};
        const long long K = (long long)B * Hout * Wout, nx = (long long)B * Hin * Win * Cin;
        const long long kend = (K + 31) / 32 * 32 + 32;
        const long long before = fails;
        for (int tap = 0; tap < k * k; ++tap) {
            const int kh = tap / k, kw = tap % k;
            long long hits = 0;
            for (long long p = 0; p < kend; ++p) {
                const long long off = conv_wgrad_src(g, p, tap);
                EXPECT(off == CONV_WGRAD_ZERO || (off >= 0 && off + Cin <= nx && off % Cin == 0), "p %lld tap %d: offset %lld outside X (%lld elements)",
                       p, tap, off, nx);
                long long want = CONV_WGRAD_ZERO;
                if (p < K) {
                    const long long b = p / ((long long)Hout * Wout), rem = p % ((long long)Hout * Wout);
                    const long long oy = rem / Wout, ox = rem % Wout;
                    const long long y = oy * stride + kh - pad, x = ox * stride + kw - pad;  // in the upsampled, unpadded input
                    if (y >= 0 && y < (long long)Hin * ups && x >= 0 && x < (long long)Win * ups)
                        want = ((b * Hin + y / ups) * Win + x / ups) * Cin;
                    if (off != CONV_WGRAD_ZERO)
                        EXPECT(off / ((long long)Hin * Win * Cin) == b, "p %lld tap %d: offset %lld lies in image %lld, the pixel in image %lld", p,
                               tap, off, off / ((long long)Hin * Win * Cin), b);
                }
                EXPECT(off == want, "p %lld tap %d: offset %lld, the definition gives %lld", p, tap, off, want);
                hits += off != CONV_WGRAD_ZERO;
            }
            const long long closed = (long long)B * count_axis(Hout, stride, kh, pad, Hin * ups) * count_axis(Wout, stride, kw, pad, Win * ups);
            EXPECT(hits == closed, "tap %d: %lld contributing pixels, closed form %lld", tap, hits, closed);
        }
        EXPECT(conv_wgrad_src(g, -1, 0) == CONV_WGRAD_ZERO, "a negative k-row must read the zero page");
        std::printf("geometry (%d,%d,%d,%d,%s,%d,%d,%d): Hout x Wout %d x %d, %lld k-rows x %d taps: %s\n", B, Hin, Win, Cin, argv[a + 4], k,
                    stride, ups, Hout, Wout, kend, k * k, fails == before ? "ok" : "FAILED");
    }
    return fails ? 1 : 0;
}
