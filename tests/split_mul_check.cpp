// Host check of the split encode's arithmetic (csrc/rs_gf.hpp gf_half_mul and the
// butterflies built from it, csrc/rs_mono.hip split_layer0), compiled together with
// csrc/gf_tables.cpp and run by tests/test_split_mul_cpu.py.  The device functions are
// written out again in plain C++ with v_perm_b32 emulated, lane pairs as two values:
//   - for random multipliers and words, the low-plane lane's (own, other) and the
//     high-plane lane's combine to exactly gf_muladd4's result, which is the field
//     product of every element (GfTables::mul);
//   - the IFFT and FFT butterflies of the two lanes equal ifft_bfly / fft_bfly;
//   - layer 0 on a pair row's plane words equals ifft_bfly2 / fft_bfly2 on the two rows,
//     on either lane of the pair.
// The halves of a table are taken through rs_stage_map.hpp SplitImage::plane_word, the
// map the staged images are built with.
#include <cstdint>
#include <cstdio>

#include "gf_tables.hpp"
#include "rs_stage_map.hpp"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (g_fail++ < 20) {                 \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

// v_perm_b32 D, S0, S1, SEL: selector byte 0-3 picks S1's byte, 4-7 S0's, 0x0C gives 0
uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    const uint64_t src = (uint64_t(s0) << 32) | s1;
    uint32_t d = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t v = (sel >> (8 * i)) & 0xFFu;
        const uint32_t byte = v < 8 ? uint32_t(src >> (8 * v)) & 0xFFu : 0u;
        d |= byte << (8 * i);
    }
    return d;
}
uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }

// rs_gf.hpp gf_muladd4
void gf_muladd4(uint32_t &acc_l, uint32_t &acc_h, uint32_t xl, uint32_t xh, const uint32_t *t) {
    const uint64_t x = (uint64_t(xh) << 32) | xl, x3 = x >> 3, x6 = x >> 6;
    const uint32_t l0 = xl & 0x07070707u, l1 = uint32_t(x3) & 0x07070707u, l2 = uint32_t(x6) & 0x03030303u;
    const uint32_t h0 = xh & 0x07070707u, h1 = uint32_t(x3 >> 32) & 0x07070707u, h2 = uint32_t(x6 >> 32) & 0x03030303u;
    acc_l = xor3(acc_l, xor3(perm(t[1], t[0], l0), perm(t[3], t[2], l1), perm(t[4], t[4], l2)),
                 xor3(perm(t[11], t[10], h0), perm(t[13], t[12], h1), perm(t[14], t[14], h2)));
    acc_h = xor3(acc_h, xor3(perm(t[6], t[5], l0), perm(t[8], t[7], l1), perm(t[9], t[9], l2)),
                 xor3(perm(t[16], t[15], h0), perm(t[18], t[17], h1), perm(t[19], t[19], h2)));
}
// rs_gf.hpp gf_muladd2 (x = [lo0 lo1 hi0 hi1], 16-word table)
void gf_muladd2(uint32_t &acc, uint32_t x, const uint32_t *t) {
    const uint32_t xr = (x >> 16) | (x << 16);
    const uint64_t xx = (uint64_t(xr) << 32) | x;
    auto sel = [](uint32_t v) { return (v & 0x03030303u) | 0x04040000u; };
    uint32_t r = acc;
    for (int f = 0; f < 4; ++f) {
        const uint64_t s = xx >> (2 * f);
        r ^= perm(t[4 * f + 1], t[4 * f], sel(uint32_t(s))) ^ perm(t[4 * f + 3], t[4 * f + 2], sel(uint32_t(s >> 32)));
    }
    acc = r;
}

// rs_gf.hpp gf_half_mul: one lane, its plane's word x and its ten words h
void gf_half_mul(uint32_t x, const uint32_t *h, uint32_t &own, uint32_t &other) {
    const uint32_t m7 = 0x07070707u, m3 = 0x03030303u;
    const uint32_t s0 = x & m7, s1 = (x >> 3) & m7, s2 = (x >> 6) & m3;
    own = xor3(perm(h[1], h[0], s0), perm(h[3], h[2], s1), perm(h[4], h[4], s2));
    other = xor3(perm(h[6], h[5], s0), perm(h[8], h[7], s1), perm(h[9], h[9], s2));
}
// a lane pair: v[0] the even (low-plane) lane's value, v[1] the odd lane's
struct Pair {
    uint32_t v[2];
};
// rs_gf.hpp gf_half_muladd on both lanes of a pair (the DPP XOR: the other lane's `other`)
void gf_half_muladd(Pair &acc, const Pair &x, const uint32_t (&h)[2][10]) {
    uint32_t own[2], other[2];
    for (int p = 0; p < 2; ++p) gf_half_mul(x.v[p], h[p], own[p], other[p]);
    for (int p = 0; p < 2; ++p) acc.v[p] ^= other[p ^ 1] ^ own[p];
}

uint32_t rnd() {
    static uint64_t s = 0x9E3779B97F4A7C15ull;
    s ^= s << 13, s ^= s >> 7, s ^= s << 17;
    return uint32_t(s >> 16);
}

}  // namespace

int main() {
    const rs::GfTables &T = rs::tables();
    using SI = rs::SplitImage<10>;
    for (int it = 0; it < 4000; ++it) {
        // multipliers: random logs, and the corners (1, the zero table of skew 65535)
        const uint32_t lm = it == 0 ? 0u : it == 1 ? 65535u : rnd() & 0xFFFFu;
        const bool zero = it == 2;
        const uint32_t *t = zero ? &T.perm_by_skew[size_t(65535) * rs::kPermWords] : &T.perm_by_log[size_t(lm) * rs::kPermWords];
        const uint32_t *t2 = zero ? &T.perm2_by_skew[size_t(65535) * rs::kPerm2Words] : &T.perm2_by_log[size_t(lm) * rs::kPerm2Words];
        auto mul = [&](uint16_t x) { return zero ? uint16_t(0) : T.mul(x, uint16_t(lm)); };
        uint32_t h[2][10];
        for (uint32_t w = 0; w < 20; ++w) h[w / 10][w % 10] = t[SI::plane_word(w)];
        const uint32_t xl = rnd(), xh = rnd(), al = rnd(), ah = rnd();
        // the quarters
        uint32_t rl = 0, rh = 0;
        gf_muladd4(rl, rh, xl, xh, t);
        for (int e = 0; e < 4; ++e) {
            const uint16_t x = uint16_t(((xl >> (8 * e)) & 0xFF) | (((xh >> (8 * e)) & 0xFF) << 8));
            const uint16_t p = uint16_t(((rl >> (8 * e)) & 0xFF) | (((rh >> (8 * e)) & 0xFF) << 8));
            CHECK(p == mul(x), "gf_muladd4 element %d of it %d", e, it);
        }
        uint32_t own[2], other[2];
        gf_half_mul(xl, h[0], own[0], other[0]);
        gf_half_mul(xh, h[1], own[1], other[1]);
        CHECK((own[0] ^ other[1]) == rl && (own[1] ^ other[0]) == rh, "halves of it %d (log %u)", it, lm);
        // butterflies
        for (int fft = 0; fft < 2; ++fft) {
            uint32_t a_l = al, a_h = ah, b_l = xl, b_h = xh;
            Pair a{{al, ah}}, b{{xl, xh}};
            if (fft) {
                gf_muladd4(a_l, a_h, b_l, b_h, t);
                b_l ^= a_l, b_h ^= a_h;
                gf_half_muladd(a, b, h);
                b.v[0] ^= a.v[0], b.v[1] ^= a.v[1];
            } else {
                b_l ^= a_l, b_h ^= a_h;
                gf_muladd4(a_l, a_h, b_l, b_h, t);
                b.v[0] ^= a.v[0], b.v[1] ^= a.v[1];
                gf_half_muladd(a, b, h);
            }
            CHECK(a.v[0] == a_l && a.v[1] == a_h && b.v[0] == b_l && b.v[1] == b_h, "%s butterfly of it %d",
                  fft ? "fft" : "ifft", it);
        }
        // layer 0: pair row (rows A, B), planes X = [A.lo0 A.lo1 B.lo0 B.lo1], Y = the high bytes
        for (int fft = 0; fft < 2; ++fft) {
            const uint32_t X = xl, Y = xh;
            uint32_t ra = perm(Y, X, 0x05040100u), rb = perm(Y, X, 0x07060302u);  // rows' words [lo0 lo1 hi0 hi1]
            if (fft) {
                gf_muladd2(ra, rb, t2);
                rb ^= ra;
            } else {
                rb ^= ra;
                gf_muladd2(ra, rb, t2);
            }
            // against the field: row A' = A ^ m * (A ^ B) (IFFT), A' = A ^ m * B (FFT)
            for (int e = 0; e < 2; ++e) {
                const uint16_t A = uint16_t(((X >> (8 * e)) & 0xFF) | (((Y >> (8 * e)) & 0xFF) << 8));
                const uint16_t B = uint16_t(((X >> (16 + 8 * e)) & 0xFF) | (((Y >> (16 + 8 * e)) & 0xFF) << 8));
                const uint16_t A2 = fft ? uint16_t(A ^ mul(B)) : uint16_t(A ^ mul(uint16_t(A ^ B)));
                const uint16_t B2 = fft ? uint16_t(B ^ A2) : uint16_t(A ^ B);
                const uint16_t ga = uint16_t(((ra >> (8 * e)) & 0xFF) | (((ra >> (16 + 8 * e)) & 0xFF) << 8));
                const uint16_t gb = uint16_t(((rb >> (8 * e)) & 0xFF) | (((rb >> (16 + 8 * e)) & 0xFF) << 8));
                CHECK(ga == A2 && gb == B2, "2-element layer 0 (%s) element %d of it %d", fft ? "fft" : "ifft", e, it);
            }
            const uint32_t wantX = perm(rb, ra, 0x05040100u), wantY = perm(rb, ra, 0x07060302u);
            for (int hp = 0; hp < 2; ++hp) {  // rs_mono.hip split_layer0 on the even and on the odd lane
                const uint32_t self = hp ? Y : X, nb = hp ? X : Y;
                const uint32_t sel_a = hp ? 0x01000504u : 0x05040100u, sel_b = hp ? 0x03020706u : 0x07060302u;
                const uint32_t sel_o = hp ? 0x07060302u : 0x05040100u;
                uint32_t a = perm(nb, self, sel_a), b = perm(nb, self, sel_b);
                if (fft) {
                    gf_muladd2(a, b, t2);
                    b ^= a;
                } else {
                    b ^= a;
                    gf_muladd2(a, b, t2);
                }
                CHECK(perm(b, a, sel_o) == (hp ? wantY : wantX), "split layer 0 (%s) lane %d of it %d", fft ? "fft" : "ifft",
                      hp, it);
            }
        }
    }
    if (g_fail) {
        std::printf("split mul: %d checks failed\n", g_fail);
        return 1;
    }
    std::printf("split mul ok\n");
    return 0;
}
