// TIFF movies in: sprk_tiff_decode (`joint align` on .tif / .tiff).
//
// One launch per frame: the frame's strips, as they lie in the file, to the [ny, nx] sample block every other kernel takes.
// One wave decodes one strip; include/sprk.h states what it computes.  How:
//
// * A code's string is always a contiguous range of the strip's output that has been written already: the string of a new
//   code is the previous string plus one byte, and those were just written next to each other.  So the table holds no prefix
//   chain.  Entry c is one position: where its string starts in the strip's output.  The length is not stored: entry c was
//   made when the string after it began, so len(c) = pos(c + 1) - pos(c) + 1 (`lastnext` stands in for pos(c + 1) of the
//   newest entry).  4096 x 4 bytes = 16 KiB of LDS per wave.
// * The newest 16 KiB of the strip's output are mirrored in LDS, a ring indexed by the position modulo its size.  Emitting a
//   code is a wave-wide copy, lane l taking bytes l, 64 + l, ...: from the ring when the whole source still lies in it, from
//   the output in global memory otherwise, into the ring and into the output.  In the "code == next free" case the last
//   byte is the string's own first byte.  With libtiff's Clear at 4094 entries, 99 % of the strings of Poisson counts longer
//   than four bytes start within the last 16 KiB (measured with the model encoder); a writer that never clears reaches
//   further back, through global memory.  (Measured, DESIGN §4.3o: the ring is worth 3 to 9 % against copying inside the
//   output; what a code costs is the serial parse, 0.3 us before anything is copied.)
// * 32 KiB per wave, 64 KiB per workgroup of two waves: two workgroups, four waves (one per SIMD) on a compute unit of 160 KiB.
// * A wave's stores and later loads of the same bytes by other lanes go through the vector memory path in program order
//   (one wave, one queue), and its LDS operations likewise; the wavefront fences keep the compiler from moving them.  Nothing
//   but this wave touches the strip's output range.
// * Only the parse is serial, and it is uniform across the wave: the input is held as 64 big-endian dwords, one per lane
//   (256 bytes, the next 256 already in flight), a dword is taken out with readlane into a 64-bit bit buffer, and the table
//   reads go through readfirstlane, so that the state (bit buffer, width, next free code, positions) stays in scalar
//   registers and the branches on it are scalar branches.
//
// No atomics, no workspace, no host synchronisation.
#include <cstdint>

#include "common.h"

namespace {

constexpr int kMaxStrips = 1 << 20;
constexpr int kWaves = 2;                        // per workgroup: 2 x (16 KiB of table + 16 KiB of ring)
constexpr int kTable = 4096;
constexpr int kRing = 16384;                     // bytes of the strip's newest output mirrored in LDS (a power of two)
constexpr int kClear = 256, kEoi = 257, kFirst = 258;

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ long uni64(long v) {
    return (long)(((uint64_t)uni((uint32_t)((uint64_t)v >> 32)) << 32) | uni((uint32_t)v));
}
__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long lmax(long a, long b) { return a > b ? a : b; }
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the big-endian dword of src at byte a (a % 4 == 0, a >= 0): bytes at or past `nbytes` read as 0 and are never touched
__device__ __forceinline__ uint32_t load_be32(const uint8_t *__restrict__ src, long a, long nbytes) {
    if (a + 4 <= nbytes) return __builtin_bswap32(*reinterpret_cast<const uint32_t *>(src + a));
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j)
        if (a + j < nbytes) w |= (uint32_t)src[a + j] << (24 - 8 * j);
    return w;
}

// the output element of decoded byte i: the byte itself, or (widen) one little-endian uint16 holding it
template <typename E>
__device__ __forceinline__ void put(E *out, long i, uint32_t b) { out[i] = (E)b; }
template <typename E>
__device__ __forceinline__ uint32_t get(const E *out, long i) { return (uint32_t)out[i] & 255u; }

// grid ceil(n_strips / kWaves), kWaves * 64 threads; E = uint8_t, or uint16_t with widen
template <typename E>
__global__ __launch_bounds__(kWaves * 64) void tiff_decode_kernel(const uint8_t *__restrict__ src, long nbytes,
                                                                  const long *__restrict__ strip_off,
                                                                  const long *__restrict__ strip_len,
                                                                  const long *__restrict__ strip_out, int n_strips,
                                                                  int compression, E *out, long out_elems, int *status) {
    __shared__ uint32_t tables[kWaves][kTable];
    __shared__ uint8_t rings[kWaves][kRing];
    const int lane = threadIdx.x & 63;
    const int wave = (int)uni(threadIdx.x >> 6);
    const int s = blockIdx.x * kWaves + wave;
    if (s >= n_strips) return;
    uint32_t *tab = tables[wave];
    uint8_t *ring = rings[wave];

    // where the strip's output starts: the sum of the strips before it, every term clamped as this strip's own is
    long before = 0;
    for (int t = lane; t < s; t += 64) before += lmin(lmax(strip_out[t], 0L), out_elems);
    for (int d = 32; d; d >>= 1) before += __shfl_xor(before, d);
    const long obase = uni64(lmin(before, out_elems));
    const uint32_t so = (uint32_t)uni64(lmin(lmin(lmax(strip_out[s], 0L), out_elems - obase), 0x7fffffffL));
    // the strip's bytes: [lo, hi) clamped into [0, nbytes)
    const long off = uni64(strip_off[s]), len = uni64(strip_len[s]);
    const long lo = lmin(lmax(off, 0L), nbytes);
    const long hi = (len <= 0) ? lo : ((off >= nbytes - len) ? nbytes : lmax(off + len, lo));
    E *o = out + obase;
    uint32_t n = 0;                              // decoded bytes out so far
    int st = 0;

    if (compression == 1) {
        const uint32_t have = (uint32_t)lmin((long)so, hi - lo);
        for (uint32_t i = lane; i < have; i += 64) put(o, i, src[lo + i]);
        n = have;
        if (have < so) st = 2;
    } else {
        // ---- the input window ----
        const long abase = lo & ~3L;
        long chunk = abase;                      // byte address of the chunk after `nxt`
        auto load_chunk = [&](long base) -> uint32_t {
            const long a = base + 4 * lane;
            return a < hi ? load_be32(src, a, nbytes) : 0u;
        };
        uint32_t cur = load_chunk(chunk);
        uint32_t nxt = load_chunk(chunk + 256);
        chunk += 512;
        uint32_t idx = 0;                        // the next dword of `cur`
        uint64_t acc = 0;
        uint32_t have = 0;                       // valid low bits of acc
        long remain = (hi - lo) * 8;             // bits of the strip not yet taken
        auto refill = [&]() {
            acc = (acc << 32) | (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)idx);
            have += 32;
            if (++idx == 64) {
                idx = 0;
                cur = nxt;
                nxt = load_chunk(chunk);
                chunk += 256;
            }
        };
        refill();
        have -= (uint32_t)(lo - abase) * 8;

        uint32_t width = 9, next = kFirst;
        bool has_prev = false;
        uint32_t ppos = 0, plen = 0;             // the previous string: start and length
        uint32_t lastnext = 0;                   // where the string began whose emission made entry next - 1
        while (n < so) {
            if (remain < (long)width) { st = 2; break; }
            if (have < width) refill();
            const uint32_t code = (uint32_t)(acc >> (have - width)) & ((1u << width) - 1u);
            have -= width;
            remain -= width;
            if (code == kClear) {
                width = 9;
                next = kFirst;
                has_prev = false;
                continue;
            }
            if (code == kEoi) { st = 2; break; }
            uint32_t spos = 0, L = 1;
            bool kwk = false;
            if (!has_prev) {
                if (code > 255) { st = 1; break; }
            } else if (code >= kFirst) {
                if (code < next) {
                    spos = uni(tab[code]);
                    const uint32_t pn = (code + 1 == next) ? lastnext : uni(tab[(code + 1) & (kTable - 1)]);
                    L = pn - spos + 1;
                } else if (code == next) {
                    kwk = true;
                    spos = ppos;
                    L = plen + 1;
                } else {
                    st = 1;
                    break;
                }
            }
            const uint32_t Lw = min(L, so - n);
            if (code < 256) {
                if (lane == 0) {
                    ring[n & (kRing - 1)] = (uint8_t)code;
                    put(o, (long)n, code);
                }
            } else {
                // the source [spos, spos + L) ends at or before n; it is still in the ring when none of it is older than
                // kRing bytes before the end of what this code writes (the writes of this code then overwrite none of it)
                const bool near = (long)spos >= (long)n + Lw - kRing;
                for (uint32_t i = lane; i < Lw; i += 64) {
                    const uint32_t sp = spos + ((kwk && i == L - 1) ? 0u : i);
                    const uint32_t b = near ? (uint32_t)ring[sp & (kRing - 1)] : get(o, (long)sp);
                    ring[(n + i) & (kRing - 1)] = (uint8_t)b;
                    put(o, (long)n + i, b);
                }
            }
            wave_fence();
            if (Lw < L) {
                n += Lw;
                st = 3;
                break;
            }
            if (has_prev && next < kTable) {
                tab[next] = ppos;                            // every lane the same value: no branch, one LDS write
                ++next;
                lastnext = n;
                if (next == 511 || next == 1023 || next == 2047) ++width;
            }
            has_prev = true;
            ppos = n;
            plen = L;
            n += L;
        }
    }
    for (uint32_t i = n + lane; i < so; i += 64) put(o, i, 0u);
    if (lane == 0) status[s] = st;
}

}  // namespace

extern "C" int sprk_tiff_decode(const uint8_t *src, long nbytes, const long *strip_off, const long *strip_len,
                                const long *strip_out, int n_strips, int compression, int widen, void *out, long out_elems,
                                int *status, void *stream) {
    SPRK_REQUIRE(src && strip_off && strip_len && strip_out && out && status, "tiff_decode: null pointer");
    SPRK_REQUIRE(1 <= nbytes, "tiff_decode: %ld bytes of strips (at least 1)", nbytes);
    SPRK_REQUIRE(1 <= n_strips && n_strips <= kMaxStrips, "tiff_decode: %d strips (1..%d)", n_strips, kMaxStrips);
    SPRK_REQUIRE(compression == 1 || compression == 5, "tiff_decode: compression %d (1: stored, 5: LZW)", compression);
    SPRK_REQUIRE(widen == 0 || widen == 1, "tiff_decode: widen %d (0 or 1)", widen);
    SPRK_REQUIRE(1 <= out_elems, "tiff_decode: an output of %ld decoded bytes (at least 1)", out_elems);
    SPRK_REQUIRE(sprk::aligned16(src, out) && (((uintptr_t)strip_off | (uintptr_t)strip_len | (uintptr_t)strip_out) & 7) == 0 &&
                     ((uintptr_t)status & 3) == 0,
                 "tiff_decode: src and out must start 16-byte aligned, the strip tables 8-byte and status 4-byte aligned");
    SPRK_REQUIRE((const void *)src != out, "tiff_decode: out must not be src");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(sprk::cdiv(n_strips, kWaves)), block(kWaves * 64);
    if (widen)
        hipLaunchKernelGGL(tiff_decode_kernel<uint16_t>, grid, block, 0, s, src, nbytes, strip_off, strip_len, strip_out,
                           n_strips, compression, (uint16_t *)out, out_elems, status);
    else
        hipLaunchKernelGGL(tiff_decode_kernel<uint8_t>, grid, block, 0, s, src, nbytes, strip_off, strip_len, strip_out, n_strips,
                           compression, (uint8_t *)out, out_elems, status);
    return sprk::check_launch("tiff_decode");
}
