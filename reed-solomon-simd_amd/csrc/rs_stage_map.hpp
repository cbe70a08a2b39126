// Slot maps of the column kernel's staged twiddle tables (rs_mono.hip Stage / LdsTabs).
//
// A staged region is a run of 20-word LDS slots, one table per slot.  The forward maps
// (sg, sq, at*) say where image piece q of a region goes: they serve the register-staged
// fill (global_load_dwordx4, then ds_write_b128 at at*(q)) and every table read.  The
// inverse maps (inv*) say which image piece belongs at 16-byte position p of a region:
// they serve the LDS-DMA fill (RS_MONO_LDS_DMA), whose destination is linear -- lane l
// of DMA instruction kc fills position 64 kc + l -- so the permutation goes on the
// source address.  Plain constexpr functions: the kernel and a host test
// (tests/test_stage_map_cpu.py) compile the same text.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RS_SM_FN __host__ __device__ __forceinline__ constexpr
#else
#define RS_SM_FN inline constexpr
#endif

namespace rs {

// floor(log2 v), v >= 1
RS_SM_FN uint32_t sm_log2(uint32_t v) { return 31u - uint32_t(__builtin_clz(v)); }

// Geometry of a staged kernel variant: 2^L rows, 2^IW rows per wave, FLO the lowest FFT
// layer of the top placement (Plan::FLO), B0 = 1 when layer 0 of phases 1 and 3 takes
// turns with the layers above in the wave regions, E elements per pack.
template <int L, int IW, int FLO, int B0, int E>
struct StageMap {
    static_assert(E == 4 || E == 2, "pack format");
    static constexpr uint32_t PC = E == 4 ? 5 : 4;  // 16-byte pieces per table
    static constexpr uint32_t SPC = 5;              // 16-byte pieces per slot (20 words)
    static constexpr bool kGray = E == 2;
    static constexpr uint32_t n = 1u << L, W = 1u << IW;
    static constexpr bool kTop = L > IW;  // wave bits: a shared region, two segments
    static constexpr int NB3 = kTop ? FLO : L;
    static constexpr uint32_t kUp = (W >> B0) - 1;          // tables of phase 1 (layer 0 apart)
    static constexpr uint32_t kP3 = (W >> B0) - (W >> NB3);  // tables of phase 3 (layer 0 apart)
    static constexpr uint32_t kL0 = W >> 1;                 // layer-0 tables of a wave region
    static constexpr uint32_t kPriv = B0 ? (W >> 1) : W - 1;  // slots of a wave region
    static constexpr uint32_t kShI = kTop ? (n >> IW) - 1 : 0;
    static constexpr uint32_t kShF = kTop ? (n >> FLO) - 1 : 0;
    static constexpr uint32_t kShared = kShI + kShF;
    static constexpr uint32_t kImgTabs = n - 1;  // tables of a layer-ordered image
    static constexpr uint32_t kSeq = IW - B0;    // a wave region's layers hold 2^kSeq - 1 tables

    // ---- forward: table -> slot -------------------------------------------------------
    // Within a layer, group g's table sits at slot sg(g) of the layer's range
    static RS_SM_FN uint32_t sg(uint32_t g) { return kGray ? g ^ ((g >> 1) & 15u) : g; }
    // 2^m - 1 for the layer (of 2^m tables) that holds table or slot t of a sequence of
    // 2^k - 1 tables, layers largest first (the layer of size 2^m starts at 2^k - 2^(m+1),
    // a multiple of 2^m; sq permutes inside a layer, so a table and its slot agree)
    static RS_SM_FN uint32_t layer_mask(uint32_t t, uint32_t k) {
        const uint32_t y = (1u << k) - t;  // 2^m < y <= 2^(m+1)
        return y <= 1u ? 0u : (1u << sm_log2(y - 1u)) - 1u;
    }
    // slot of table t of such a sequence
    static RS_SM_FN uint32_t sq(uint32_t t, uint32_t k) {
        if constexpr (!kGray) return t;
        const uint32_t mask = layer_mask(t, k);
        return t ^ (((t & mask) >> 1) & 15u);
    }
    // LDS position (16-byte units) of image piece q: slot f(q / PC), piece q % PC
    template <typename F>
    static RS_SM_FN uint32_t at(uint32_t q, F f) {
        const uint32_t t = q / PC;
        return f(t) * SPC + (q - t * PC);
    }
    // the phase-1 / -3 region (layers B0..IW-1), its layer-0 turn (B0), the shared region
    // (IFFT layers IW..L-1, then FFT layers FLO..L-1, then any further tables in order)
    static RS_SM_FN uint32_t at1(uint32_t q) {
        return at(q, [](uint32_t t) { return sq(t, kSeq); });
    }
    static RS_SM_FN uint32_t at0(uint32_t q) {
        return at(q, [](uint32_t t) { return sg(t); });
    }
    static RS_SM_FN uint32_t atS(uint32_t q) {
        return at(q, [](uint32_t t) {
            if (t < kShI) return sq(t, uint32_t(L - IW));
            if (t < kShI + kShF) return kShI + sq(t - kShI, uint32_t(L - FLO));
            return t;
        });
    }

    // ---- inverse: slot -> table -------------------------------------------------------
    // sg flips bit i < 4 of g by bit i + 1: a Gray code on the low 5 bits, bit 4 fixed.
    // Its inverse is the prefix XOR from bit 4 down: g = h ^ P((h >> 1) & 15) with
    // P(z) = z ^ z >> 1 ^ z >> 2 ^ z >> 3
    static RS_SM_FN uint32_t gray_fix(uint32_t z) {
        const uint32_t a = z ^ (z >> 1);
        return a ^ (a >> 2);
    }
    static RS_SM_FN uint32_t sg_inv(uint32_t h) { return kGray ? h ^ gray_fix((h >> 1) & 15u) : h; }
    // table at slot s of a sequence, `mask` its layer's (layer_mask(s, k))
    static RS_SM_FN uint32_t sq_inv_mask(uint32_t s, uint32_t mask) {
        if constexpr (!kGray) return s;
        return s ^ gray_fix(((s & mask) >> 1) & 15u);
    }
    static RS_SM_FN uint32_t sq_inv(uint32_t s, uint32_t k) { return sq_inv_mask(s, layer_mask(s, k)); }

    // A fill position's source: a table of the region and one of its pieces; real = false
    // for a slot's padding (2-element packs: piece 4 of a slot, which nothing reads), which
    // names the table's last piece -- a valid address on the line its neighbours fetch.
    struct Src {
        uint32_t t, piece;  // table of the region and its piece: q = t * PC + piece
        bool real;
    };
    template <typename F>
    static RS_SM_FN Src inv(uint32_t p, F table_at) {
        const uint32_t s = p / SPC, piece = p - s * SPC;
        const bool real = piece < PC;
        return Src{table_at(s), real ? piece : PC - 1u, real};
    }
    static RS_SM_FN Src inv1(uint32_t p) {
        return inv(p, [](uint32_t s) { return sq_inv(s, kSeq); });
    }
    // inv1 where the caller knows the layer mask of the position's slot (a DMA instruction
    // whose 64 positions lie in one layer: the mask is a compile-time constant)
    static RS_SM_FN Src inv1_mask(uint32_t p, uint32_t mask) {
        return inv(p, [mask](uint32_t s) { return sq_inv_mask(s, mask); });
    }
    static RS_SM_FN Src inv0(uint32_t p) {
        return inv(p, [](uint32_t s) { return sg_inv(s); });
    }
    static RS_SM_FN Src invS(uint32_t p) {
        return inv(p, [](uint32_t s) {
            if (s < kShI) return sq_inv(s, uint32_t(L - IW));
            if (s < kShI + kShF) return kShI + sq_inv(s - kShI, uint32_t(L - FLO));
            return s;
        });
    }

    // ---- region piece -> image piece (16-byte units; LPC image pieces per table) --------
    // layer of table t of a wave region (phases 1 and 3)
    static RS_SM_FN uint32_t priv_layer(uint32_t t) {
        const uint32_t y = (W >> B0) - t;  // in [2, W >> B0]: the region has (W >> B0) - 1 tables
        return uint32_t(IW - int(32 - __builtin_clz(y - 1)));  // IW - ceil(log2 y)
    }
    // image table of table t (layer b) of wave `wave`'s region
    static RS_SM_FN uint32_t priv_table(uint32_t wave, uint32_t t, uint32_t b) {
        const uint32_t local = t - ((W >> B0) - (W >> b));
        return n - (n >> b) + wave * (W >> (b + 1)) + local;
    }
    // the same from the layer's mask (layer_mask: the layer holds S = mask + 1 tables, so
    // W >> b = 2 S and n >> b = 2 S n / W): t + n - (W >> B0) - S (2 n / W - 2 - wave),
    // one multiply-add per lane beside wave-uniform terms
    static RS_SM_FN uint32_t priv_table_mask(uint32_t wave, uint32_t t, uint32_t mask) {
        return t + (n - (W >> B0)) - (mask + 1u) * (2u * (n / W) - 2u - wave);
    }
    static RS_SM_FN uint32_t priv_index(uint32_t wave, uint32_t q, uint32_t LPC = PC) {
        const uint32_t t = q / LPC, piece = q - t * LPC;
        return priv_table(wave, t, priv_layer(t)) * LPC + piece;
    }
    // layer-0 tables of wave `wave`'s rows: image slots wave * W/2 .. (contiguous)
    static RS_SM_FN uint32_t l0_index(uint32_t wave, uint32_t q, uint32_t LPC = PC) {
        return wave * kL0 * LPC + q;
    }
    // shared region: from_fft says which image (IFFT part first)
    static RS_SM_FN bool shared_from_fft(uint32_t q, uint32_t LPC = PC) { return q / LPC >= kShI; }
    static RS_SM_FN uint32_t shared_table(uint32_t t) {  // image table of shared table t
        return t < kShI ? n - (n >> IW) + t : n - (n >> FLO) + (t - kShI);
    }
    static RS_SM_FN uint32_t shared_index(uint32_t q, uint32_t LPC = PC) {
        const uint32_t t = q / LPC, piece = q - t * LPC;
        return shared_table(t) * LPC + piece;
    }

    // ---- DMA fills: instruction counts (64 positions each) ------------------------------
    static constexpr uint32_t insts(uint32_t tables) { return (tables * SPC + 63u) / 64u; }
};

// The staged single-chunk encodes (2^7..2^11 rows, 2 rows per lane: IW = 7; the FFT
// leaves the top placement after layer IW; layer 0 takes turns at 2^11 rows)
template <int L, int E>
using EncodeStageMap = StageMap<L, 7, (L > 7 ? 7 : 0), (L >= 11 ? 1 : 0), E>;

// The split encode's images (rs_mono.hip k_mono_split: the two byte planes of a pair
// row on neighbouring lanes).  Regions, slots and the Gray swizzle are EncodeStageMap<L, 2>'s;
// the contents differ: layer 0's tables stay 2-element tables (16 words + padding), the
// layers above are 4-element tables (20 words, rs_gf.hpp gf_muladd4: rows 2q and 2q + 1
// share every twiddle above row bit 0), each as the two planes' halves: slot words 0-9
// the low-plane lane's (table words 0-9: own quarter, then the neighbour's), slot words
// 10-19 the high-plane lane's (table words 15-19, then 10-14: own quarter first again,
// rs_gf.hpp gf_half_mul).  One image per skew offset is kept in the order the LDS-DMA
// fill wants -- wave 0's region, ..., the last wave's, then the 2^(L-IW) - 1 tables of
// layers IW..L-1 as the shared region holds them -- so a fill position's source is the
// position itself: no inverse map on the device.  The host builds the image from
// these maps (rs_codec.cpp split_images); tests/split_plan_check.cpp walks them.
template <int L>
struct SplitImage {
    using SM = EncodeStageMap<L, 2>;
    static_assert(SM::kTop && SM::kPriv == SM::W - 1 && SM::kShI == SM::kShF && SM::kP3 == SM::kUp,
                  "split encode: wave bits, no layer-0 turns, both transforms' top tables alike");
    static constexpr uint32_t SW = 4u * SM::SPC;          // words per slot
    static constexpr uint32_t kWaves = SM::n / SM::W;
    static constexpr uint32_t kPrivWords = SM::kPriv * SW;  // a wave region
    static constexpr uint32_t kTop = SM::kShI;            // tables of layers IW..L-1
    static constexpr uint32_t kWords = (kWaves * SM::kPriv + kTop) * SW;  // one image
    static RS_SM_FN uint32_t priv_off(uint32_t wave) { return wave * kPrivWords; }  // (words)
    static RS_SM_FN uint32_t top_off() { return kWaves * kPrivWords; }
    // 16-byte positions of a wave region's fill, of one transform's part of the shared region
    static constexpr uint32_t kPrivPos = SM::kPriv * SM::SPC, kTopPos = kTop * SM::SPC;
    // A slot word's source: word `word` of table `table` of the layer-ordered image of
    // `elems`-element tables (rs_device.hpp: slot n - n / 2^b + g); elems = 0: padding
    struct Word {
        uint32_t elems, table, word;
    };
    // slot word w of a 4-element table -> table word
    static RS_SM_FN uint32_t plane_word(uint32_t w) { return w < 10u ? w : w < 15u ? w + 5u : w - 5u; }
    static RS_SM_FN Word priv_word(uint32_t wave, uint32_t slot, uint32_t w) {
        const uint32_t t = SM::sq_inv(slot, SM::kSeq), b = SM::priv_layer(t);
        const uint32_t table = SM::priv_table(wave, t, b);
        if (b == 0) return w < 16u ? Word{2u, table, w} : Word{0u, table, 0u};
        return Word{4u, table, plane_word(w)};
    }
    static RS_SM_FN Word top_word(uint32_t slot, uint32_t w) {
        return Word{4u, SM::shared_table(SM::sq_inv(slot, uint32_t(L) - SM::kSeq)), plane_word(w)};
    }
};

// Skew index of table slot `slot` of image t (skew offset t * 2^L) of a layer-ordered
// image of a 2^L-row transform (rs_device.hpp: layer b's group g at slot n - n / 2^b + g)
RS_SM_FN uint32_t image_skew_index(uint32_t L, uint32_t t, uint32_t slot) {
    const uint32_t n = 1u << L;
    uint32_t b = 0;
    while (slot >= n - (n >> (b + 1))) ++b;
    const uint32_t g = slot - (n - (n >> b));
    return (g << (b + 1)) + (1u << b) + t * n - 1u;
}

// Split image t into dst (SplitImage<L>::kWords words) from the perm tables by skew
// index, perm4: 20 words per table, perm2: 16 (gf_tables.hpp perm_by_skew / perm2_by_skew)
template <int L>
inline void split_image_fill(uint32_t *dst, uint32_t t, const uint32_t *perm4, const uint32_t *perm2) {
    using SI = SplitImage<L>;
    auto value = [&](const typename SI::Word &s) -> uint32_t {
        const size_t idx = image_skew_index(uint32_t(L), t, s.table);
        return s.elems == 4u ? perm4[idx * 20u + s.word] : s.elems == 2u ? perm2[idx * 16u + s.word] : 0u;
    };
    for (uint32_t wave = 0; wave < SI::kWaves; ++wave)
        for (uint32_t slot = 0; slot < SI::SM::kPriv; ++slot)
            for (uint32_t w = 0; w < SI::SW; ++w)
                dst[SI::priv_off(wave) + slot * SI::SW + w] = value(SI::priv_word(wave, slot, w));
    for (uint32_t slot = 0; slot < SI::kTop; ++slot)
        for (uint32_t w = 0; w < SI::SW; ++w) dst[SI::top_off() + slot * SI::SW + w] = value(SI::top_word(slot, w));
}

}  // namespace rs
