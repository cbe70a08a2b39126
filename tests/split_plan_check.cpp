// Host walk of the split encode (csrc/rs_mono.hip k_mono_split): its plan
// (csrc/rs_mono_plan.hpp Plan<10, 1, FLOW | PAIR>), its images and fills
// (csrc/rs_stage_map.hpp SplitImage) and its table reads, compiled together with
// csrc/gf_tables.cpp and run by tests/test_split_plan_cpu.py.  It checks
//   - every existing plan kind still comes out as seg_map's unpinned form gives it
//     (the pin changes nothing where it is not asked for);
//   - in every placement of both sequences every (pair row, plane) is held exactly once,
//     lane bit 0 is the plane, and no transpose or layer touches it;
//   - the fills: every position of a DMA lies inside its region, its source inside the
//     image, positions past the end sit out, and each slot word is a real table word
//     or padding no read touches;
//   - every (layer, group) table a wave reads in phases 1, 2 (both transforms' top
//     layers) and 3 lies in a region it may read and holds that layer's and group's
//     table, as the lane's plane's half;
// and then runs the whole kernel for one column pack on the host the way the 512 lanes
// do -- loads, layer 0 inside the words, transposes, remaps through the LDS plane, half
// butterflies on lane pairs, stores -- for both rates, against the plain transform
// (engine_naive.rs:43-105 by GfTables::mul).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gf_tables.hpp"
#include "rs_mono_plan.hpp"
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

using rs::kOpLayer;
using rs::kOpRemap;
using rs::kOpXpose;
using rs::Map;
using rs::Seq;

constexpr int L = 10, LR = 1, PK = 2 | 4;
constexpr uint32_t n = 1u << L, W = 128, kWaves = 8, SW = 20;
using P = rs::Plan<L, LR, PK>;
using SI = rs::SplitImage<L>;
using SM = SI::SM;
// the kernel's LDS (rs_mono.hip Stage<10, 1, PK, 2>): column plane, shared region, wave regions
constexpr uint32_t kPlaneWords = n, kSharedWords = SM::kShared * SW, kPrivWords = SM::kPriv * SW;
constexpr uint32_t kLdsWords = kPlaneWords + kSharedWords + kWaves * kPrivWords;
uint32_t shared_at() { return kPlaneWords; }
uint32_t priv_at(uint32_t wave) { return kPlaneWords + kSharedWords + wave * kPrivWords; }

// rs_mono.hip lane_rows / reg_rows / swz
uint32_t lane_rows(const Map &m, uint32_t lane, uint32_t wave) {
    uint32_t r = 0;
    for (int j = 0; j < 6; ++j) r |= ((lane >> j) & 1u) << m.lane[j];
    for (int k = 0; k < 4; ++k)
        if (m.wave[k] >= 0) r |= ((wave >> k) & 1u) << m.wave[k];
    return r;
}
uint32_t reg_rows(const Map &m, int i) {
    uint32_t r = 0;
    for (int s = 0; s < LR; ++s) r |= uint32_t((i >> s) & 1) << m.reg[s];
    return r;
}
uint32_t swz(uint32_t r) { return r ^ ((r >> 5) & 31u); }

uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    const uint64_t src = (uint64_t(s0) << 32) | s1;
    uint32_t d = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t v = (sel >> (8 * i)) & 0xFFu;
        d |= (v < 8 ? uint32_t(src >> (8 * v)) & 0xFFu : 0u) << (8 * i);
    }
    return d;
}
void gf_muladd2(uint32_t &acc, uint32_t x, const uint32_t *t) {  // rs_gf.hpp
    const uint32_t xr = (x >> 16) | (x << 16);
    const uint64_t xx = (uint64_t(xr) << 32) | x;
    auto sel = [](uint32_t v) { return (v & 0x03030303u) | 0x04040000u; };
    for (int f = 0; f < 4; ++f) {
        const uint64_t s = xx >> (2 * f);
        acc ^= perm(t[4 * f + 1], t[4 * f], sel(uint32_t(s))) ^ perm(t[4 * f + 3], t[4 * f + 2], sel(uint32_t(s >> 32)));
    }
}
void gf_half_mul(uint32_t x, const uint32_t *h, uint32_t &own, uint32_t &other) {  // rs_gf.hpp
    const uint32_t s0 = x & 0x07070707u, s1 = (x >> 3) & 0x07070707u, s2 = (x >> 6) & 0x03030303u;
    own = perm(h[1], h[0], s0) ^ perm(h[3], h[2], s1) ^ perm(h[4], h[4], s2);
    other = perm(h[6], h[5], s0) ^ perm(h[8], h[7], s1) ^ perm(h[9], h[9], s2);
}

// ---- the plans ---------------------------------------------------------------------
bool same_map(const Map &a, const Map &b) {
    bool ok = true;
    for (int s = 0; s < 3; ++s) ok = ok && a.reg[s] == b.reg[s];
    for (int j = 0; j < 6; ++j) ok = ok && a.lane[j] == b.lane[j];
    for (int k = 0; k < 4; ++k) ok = ok && a.wave[k] == b.wave[k];
    return ok;
}
// seg_map as it was before the pin (the parent's text)
Map seg_map_plain(int L_, int LR_, int lo, const int *order, int no) {
    const int IW = LR_ + 6;
    int pri[16] = {}, np = 0;
    for (int t = 0; t < no; ++t) {
        const int x = order[t];
        bool seen = x < lo || x >= lo + IW;
        for (int q = 0; q < np; ++q) seen = seen || pri[q] == x;
        if (!seen) pri[np++] = x;
    }
    for (int x = lo; x < lo + IW; ++x) {
        bool seen = false;
        for (int q = 0; q < np; ++q) seen = seen || pri[q] == x;
        if (!seen) pri[np++] = x;
    }
    const int pref[6] = {5, 4, 0, 1, 3, 2};
    Map m{};
    for (int s = 0; s < 3; ++s) m.reg[s] = s < LR_ ? pri[s] : -1;
    for (int j = 0; j < 6; ++j) m.lane[pref[j]] = pri[LR_ + j];
    int k = 0;
    for (int x = 0; x < L_; ++x)
        if (x < lo || x >= lo + IW) m.wave[k++] = x;
    for (; k < 4; ++k) m.wave[k] = -1;
    return m;
}
void check_unpinned() {
    for (int L_ = 7; L_ <= 12; ++L_)
        for (int LR_ = 1; LR_ <= 3 && LR_ + 6 <= L_; ++LR_)
            for (int lo = 0; lo + LR_ + 6 <= L_; ++lo) {
                int order[32], no = 0;
                for (int x = L_ - 1; x >= 0; x -= 2) order[no++] = x;  // some order with gaps
                for (int x = 0; x < L_; x += 3) order[no++] = x;
                CHECK(same_map(rs::seg_map(L_, LR_, lo, order, no), seg_map_plain(L_, LR_, lo, order, no)),
                      "seg_map without a pin, L %d LR %d lo %d", L_, LR_, lo);
            }
}
// a placement holds every (pair row, plane) once; the plane is lane bit 0
void check_placements(const Seq &s, const char *name) {
    for (int i = 0; i <= s.count; ++i) {
        const Map &m = s.maps[i];
        CHECK(m.lane[0] == 0, "%s placement %d: lane bit 0 holds bit %d", name, i, m.lane[0]);
        std::vector<int> seen(n, 0);
        for (uint32_t wave = 0; wave < kWaves; ++wave)
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 2; ++r) {
                    const uint32_t x = lane_rows(m, lane, wave) | reg_rows(m, r);
                    CHECK(x < n && (x & 1u) == (lane & 1u), "%s placement %d: index %u on lane %u", name, i, x, lane);
                    if (x < n) ++seen[x];
                }
        for (uint32_t x = 0; x < n; ++x) CHECK(seen[x] == 1, "%s placement %d: (pair row %u, plane %u) held %d times", name, i, x >> 1, x & 1u, seen[x]);
    }
    for (int i = 0; i < s.count; ++i) {
        const rs::Op &op = s.ops[i];
        if (op.kind == kOpXpose) CHECK(op.ls != 0 && op.bit != 0, "%s op %d: a transpose on the plane", name, i);
        if (op.kind == kOpLayer) CHECK(op.bit >= 1 && op.bit < L, "%s op %d: a layer on bit %d", name, i, op.bit);
    }
}

// ---- the kernel on the host ----------------------------------------------------------
struct Kernel {
    const rs::GfTables &T;
    std::vector<uint32_t> img;  // the split images, skew offsets 0 and n
    std::vector<uint32_t> lds;
    uint32_t c[kWaves][64][2];
    uint32_t ii, fi;
    explicit Kernel(const rs::GfTables &t) : T(t), img(size_t(2) * SI::kWords), lds(kLdsWords, 0xDEADBEEFu) {
        for (uint32_t k = 0; k < 2; ++k)
            rs::split_image_fill<L>(&img[size_t(k) * SI::kWords], k, T.perm_by_skew.data(), T.perm2_by_skew.data());
    }
    // rs_mono.hip dma_linear: POS positions at LDS word `dst` from image words at `src`
    void dma_linear(uint32_t pos, size_t src, uint32_t dst, uint32_t region_end, const char *what) {
        for (uint32_t kc = 0; kc < (pos + 63u) / 64u; ++kc)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t p = lane + 64u * kc;
                if (!(64u * kc + 63u < pos || p < pos)) continue;  // the lane sits out
                CHECK(dst + 4u * p + 4u <= region_end, "%s: position %u past the region", what, p);
                CHECK(src + 4u * p + 4u <= img.size() && (src + 4u * p) / SI::kWords == (src / SI::kWords),
                      "%s: position %u source outside its image", what, p);
                for (uint32_t q = 0; q < 4; ++q) lds[dst + 4u * p + q] = img[src + 4u * p + q];
            }
    }
    void fill_priv(uint32_t image) {
        for (uint32_t wave = 0; wave < kWaves; ++wave)
            dma_linear(SI::kPrivPos, size_t(image) * SI::kWords + SI::priv_off(wave), priv_at(wave), priv_at(wave) + kPrivWords,
                       "wave region");
    }
    void fill_shared() {
        for (uint32_t wave = 0; wave < 2; ++wave)
            dma_linear(SI::kTopPos, size_t(wave ? fi : ii) * SI::kWords + SI::top_off(), shared_at() + wave * 4u * SI::kTopPos,
                       shared_at() + kSharedWords, "shared region");
    }
    // the table of layer x, group g of image t, as a lane of plane hp reads it
    void expect_half(uint32_t t, uint32_t x, uint32_t g, uint32_t hp, const uint32_t *got, const char *what) {
        const uint32_t idx = (g << (x + 1)) + (1u << x) + t * n - 1u;
        const uint32_t *tab = &T.perm_by_skew[size_t(idx) * rs::kPermWords];
        bool ok = true;
        for (uint32_t w = 0; w < 10; ++w) ok = ok && got[w] == tab[SI::plane_word(10u * hp + w)];
        CHECK(ok, "%s: layer %u group %u plane %u reads another table", what, x, g, hp);
    }
    // rs_mono.hip LdsTabs::tab + PlaneTabs::get (ph: 1, 2, 4, 3 as phase_of)
    const uint32_t *table(int ph, uint32_t x, uint32_t row, uint32_t wave, uint32_t hp) {
        uint32_t slot, base, cap;
        if (ph == 1 || ph == 3) {
            slot = W - (W >> x) + SM::sg((row & (W - 1u)) >> (x + 1)), base = priv_at(wave), cap = SM::kPriv;
        } else if (ph == 2) {
            slot = (n >> 7) - (n >> x) + SM::sg(row >> (x + 1)), base = shared_at(), cap = SM::kShI;
        } else {
            slot = SM::kShI + (n >> 7) - (n >> x) + SM::sg(row >> (x + 1)), base = shared_at(), cap = SM::kShared;
        }
        CHECK(slot < cap && (ph != 4 || slot >= SM::kShI), "phase %d layer %u row %u: slot %u outside its region", ph, x, row, slot);
        const uint32_t *p = &lds[base + slot * SW + 10u * hp];
        expect_half(ph <= 2 ? ii : fi, x, row >> (x + 1), hp, p, ph == 1 ? "phase 1" : ph == 2 ? "phase 2 (IFFT)" : ph == 4 ? "phase 2 (FFT)" : "phase 3");
        return p;
    }
    // rs_mono.hip split_layer0
    void layer0(const Map &m, bool fft) {
        for (uint32_t wave = 0; wave < kWaves; ++wave)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                if (lane & 1u) continue;  // both lanes of the pair, from the values before
                for (int i = 0; i < 2; ++i) {
                    const uint32_t q = ((lane_rows(m, lane, wave) | reg_rows(m, i)) & (W - 1u)) >> 1;
                    const uint32_t slot = SM::sg(q);
                    CHECK(slot < SM::kL0, "layer 0: slot %u", slot);
                    const uint32_t *t = &lds[priv_at(wave) + slot * SW];
                    const uint32_t idx = ((wave * 64u + q) << 1) + 1u + (fft ? fi : ii) * n - 1u;
                    bool ok = true;
                    for (uint32_t w = 0; w < 16; ++w) ok = ok && t[w] == T.perm2_by_skew[size_t(idx) * rs::kPerm2Words + w];
                    CHECK(ok, "layer 0 (%s) wave %u pair row %u reads another table", fft ? "fft" : "ifft", wave, q);
                    const uint32_t v[2] = {c[wave][lane][i], c[wave][lane + 1][i]};
                    for (uint32_t hp = 0; hp < 2; ++hp) {
                        const uint32_t self = v[hp], nb = v[hp ^ 1];
                        const uint32_t sel_a = hp ? 0x01000504u : 0x05040100u, sel_b = hp ? 0x03020706u : 0x07060302u;
                        const uint32_t sel_o = hp ? 0x07060302u : 0x05040100u;
                        uint32_t a = perm(nb, self, sel_a), b = perm(nb, self, sel_b);
                        if (fft) {
                            gf_muladd2(a, b, t);
                            b ^= a;
                        } else {
                            b ^= a;
                            gf_muladd2(a, b, t);
                        }
                        c[wave][lane + hp][i] = perm(b, a, sel_o);
                    }
                }
            }
    }
    // rs_mono.hip run_seq
    void run(const Seq &s, bool fft, bool zero_top) {
        int ri = s.count;
        for (int i = 0; i < s.count; ++i)
            if (s.ops[i].kind == kOpRemap) ri = i;
        for (int I = 0; I < s.count; ++I) {
            const rs::Op &op = s.ops[I];
            const Map &m = s.maps[I];
            if (op.kind == kOpXpose) {  // rs_mono.hip xpose: register pair x lane bit op.ls
                for (uint32_t wave = 0; wave < kWaves; ++wave)
                    for (uint32_t lane = 0; lane < 64; ++lane)
                        if (!((lane >> op.ls) & 1u)) {
                            uint32_t &b_lo = c[wave][lane][1], &a_hi = c[wave][lane | (1u << op.ls)][0];
                            const uint32_t t = b_lo;
                            b_lo = a_hi, a_hi = t;
                        }
            } else if (op.kind == kOpRemap) {
                if (!fft) fill_priv(fi);  // issue3: phase 3's tables over phase 1's
                const Map &m2 = s.maps[I + 1];
                for (uint32_t wave = 0; wave < kWaves; ++wave)
                    for (uint32_t lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < 2; ++i) lds[swz(lane_rows(m, lane, wave) | reg_rows(m, i))] = c[wave][lane][i];
                for (uint32_t wave = 0; wave < kWaves; ++wave)
                    for (uint32_t lane = 0; lane < 64; ++lane)
                        for (int i = 0; i < 2; ++i) c[wave][lane][i] = lds[swz(lane_rows(m2, lane, wave) | reg_rows(m2, i))];
            } else {
                const int ph = fft ? (I < ri ? 4 : 3) : (I < ri ? 1 : 2);
                for (uint32_t wave = 0; wave < kWaves; ++wave)
                    for (uint32_t lane = 0; lane < 64; lane += 2) {
                        uint32_t *a[2] = {&c[wave][lane][0], &c[wave][lane + 1][0]}, *b[2] = {&c[wave][lane][1], &c[wave][lane + 1][1]};
                        if (uint32_t(op.bit) == uint32_t(L) - 1u && zero_top) {
                            for (int hp = 0; hp < 2; ++hp) *b[hp] ^= *a[hp];
                            continue;
                        }
                        const uint32_t *h[2];
                        for (uint32_t hp = 0; hp < 2; ++hp)
                            h[hp] = table(ph, uint32_t(op.bit), lane_rows(m, lane + hp, wave) | reg_rows(m, 0), wave, hp);
                        if (!fft)
                            for (int hp = 0; hp < 2; ++hp) *b[hp] ^= *a[hp];
                        uint32_t own[2], other[2];
                        for (int hp = 0; hp < 2; ++hp) gf_half_mul(*b[hp], h[hp], own[hp], other[hp]);
                        for (int hp = 0; hp < 2; ++hp) *a[hp] ^= other[hp ^ 1] ^ own[hp];
                        if (fft)
                            for (int hp = 0; hp < 2; ++hp) *b[hp] ^= *a[hp];
                    }
            }
        }
    }
    // one column pack: in[r] = the two elements of row r; t_i / t_f the transforms' images
    void encode(uint32_t t_i, uint32_t t_f, const std::vector<uint16_t> &in, std::vector<uint16_t> &out) {
        ii = t_i, fi = t_f;
        const Map &m0 = P::ifft.maps[0], &m1 = P::fft.maps[P::fft.count];
        CHECK(m0.reg[0] == 1, "the loads take row bit 1 in the register bit");
        for (uint32_t wave = 0; wave < kWaves; ++wave)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t r0 = lane_rows(m0, lane & ~1u, wave), hp = lane & 1u;
                for (uint32_t i = 0; i < 2; ++i) {
                    uint32_t word = 0;
                    for (uint32_t k = 0; k < 4; ++k)  // [row 2q e0, row 2q e1, row 2q+1 e0, row 2q+1 e1], plane hp
                        word |= uint32_t((in[2 * (r0 + 2 * i + (k >> 1)) + (k & 1u)] >> (8 * hp)) & 0xFF) << (8 * k);
                    c[wave][lane][i] = word;
                }
            }
        fill_priv(ii);
        fill_shared();
        layer0(m0, false);
        run(P::ifft, false, ii == 0);
        run(P::fft, true, fi == 0);
        layer0(m1, true);
        out.assign(2 * n, 0);
        for (uint32_t wave = 0; wave < kWaves; ++wave)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t r0 = lane_rows(m1, lane & ~1u, wave), hp = lane & 1u;
                for (uint32_t j = 0; j < 4; ++j) {  // paired_delta: (j & 1) + the register bit's rows
                    const uint32_t r = r0 + (j & 1u) + reg_rows(m1, int(j >> 1));
                    const uint32_t half = (j & 1u) ? c[wave][lane][j >> 1] >> 16 : c[wave][lane][j >> 1] & 0xFFFFu;
                    out[2 * r] |= uint16_t((half & 0xFFu) << (8 * hp));
                    out[2 * r + 1] |= uint16_t((half >> 8) << (8 * hp));
                }
            }
    }
};

// the plain transforms on one element per row
void reference(const rs::GfTables &T, uint32_t t_i, uint32_t t_f, std::vector<uint16_t> &v) {
    auto skew = [&](uint32_t t, uint32_t b, uint32_t r) { return T.skew[((r >> (b + 1)) << (b + 1)) + (1u << b) + t * n - 1u]; };
    for (uint32_t b = 0; b < uint32_t(L); ++b)
        for (uint32_t r = 0; r < n; ++r)
            if (!((r >> b) & 1u)) {
                uint16_t &x = v[r], &y = v[r + (1u << b)];
                y ^= x;
                const uint16_t lm = skew(t_i, b, r);
                if (lm != 65535) x ^= T.mul(y, lm);
            }
    for (uint32_t b = uint32_t(L); b-- > 0;)
        for (uint32_t r = 0; r < n; ++r)
            if (!((r >> b) & 1u)) {
                uint16_t &x = v[r], &y = v[r + (1u << b)];
                const uint16_t lm = skew(t_f, b, r);
                if (lm != 65535) x ^= T.mul(y, lm);
                y ^= x;
            }
}

}  // namespace

int main() {
    check_unpinned();
    check_placements(P::ifft, "ifft");
    check_placements(P::fft, "fft");
    // the image's padding: words 16-19 of a layer-0 slot, which no read touches
    for (uint32_t wave = 0; wave < kWaves; ++wave)
        for (uint32_t slot = 0; slot < SM::kPriv; ++slot)
            for (uint32_t w = 0; w < SW; ++w) {
                const auto s = SI::priv_word(wave, slot, w);
                CHECK(s.elems == (slot < SM::kL0 ? (w < 16 ? 2u : 0u) : 4u) && s.table < n - 1u && s.word < (s.elems == 2 ? 16u : 20u),
                      "wave %u slot %u word %u: source", wave, slot, w);
            }
    const rs::GfTables &T = rs::tables();
    Kernel k(T);
    uint64_t seed = 0x243F6A8885A308D3ull;
    for (int rate = 0; rate < 2; ++rate) {  // high rate: IFFT at skew offset n, FFT at 0; low rate the reverse
        const uint32_t t_i = rate == 0 ? 1 : 0, t_f = rate == 0 ? 0 : 1;
        std::vector<uint16_t> in(2 * n), out;
        for (auto &x : in) {
            seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
            x = uint16_t(seed >> 24);
        }
        k.encode(t_i, t_f, in, out);
        for (uint32_t e = 0; e < 2; ++e) {
            std::vector<uint16_t> v(n);
            for (uint32_t r = 0; r < n; ++r) v[r] = in[2 * r + e];
            reference(T, t_i, t_f, v);
            uint32_t bad = 0;
            for (uint32_t r = 0; r < n; ++r) bad += v[r] != out[2 * r + e];
            CHECK(bad == 0, "%s rate, element %u: %u of %u rows differ from the plain transform", rate ? "low" : "high", e, bad, n);
        }
    }
    if (g_fail) {
        std::printf("split plan: %d checks failed\n", g_fail);
        return 1;
    }
    std::printf("split plan ok\n");
    return 0;
}
