// Host check of the column kernel's slot maps (csrc/rs_stage_map.hpp), compiled and run
// by tests/test_stage_map_cpu.py.  For the staged encodes of 2^7..2^11 rows, both pack
// formats and every region a DMA fills (phase 1 / phase 3 tables, the layer-0 turn at
// 2^11 rows, the shared region with its IFFT and FFT parts) it walks the fill the way
// the kernel issues it -- instruction kc, lane l, position p = 64 kc + l, active while
// p lies inside the region -- and checks:
//   - position -> (table, piece) -> forward map gives the position back, and the
//     forward map of every piece inverts to that piece;
//   - every real piece of the region is produced exactly once;
//   - padding positions are pieces no table read touches (piece >= PC of a slot);
//   - every source index lies inside its image, and is the table the layer order says;
//   - no active position lies past the region (a wave's slots / the shared slots).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rs_stage_map.hpp"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (g_fail++ < 20) {              \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

// One region: N = tables * SPC positions, capacity in positions, the two maps and the
// image index of a region piece q (`want(t)`: the image table the layer order gives).
template <typename SM, typename Inv, typename At, typename Index, typename Want>
void check_region(const char *name, int L, int E, uint32_t tables, uint32_t capacity_tables, Inv inv, At at,
                  Index index, Want want) {
    const uint32_t N = tables * SM::SPC, pieces = tables * SM::PC;
    CHECK(tables <= capacity_tables, "%s L=%d E=%d: %u tables in %u slots", name, L, E, tables, capacity_tables);
    std::vector<uint32_t> count(pieces, 0);
    const uint32_t insts = SM::insts(tables);
    CHECK(insts * 64u >= N && (insts == 0 || (insts - 1u) * 64u < N), "%s L=%d E=%d: %u instructions for %u positions",
          name, L, E, insts, N);
    for (uint32_t kc = 0; kc < insts; ++kc) {
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t p = 64u * kc + lane;
            if (p >= N) continue;  // the lane sits out
            CHECK(p < capacity_tables * SM::SPC, "%s L=%d E=%d: position %u past the region", name, L, E, p);
            const auto s = inv(p);
            CHECK(s.t < tables && s.piece < SM::PC, "%s L=%d E=%d: p %u -> table %u piece %u", name, L, E, p, s.t,
                  s.piece);
            if (s.t >= tables || s.piece >= SM::PC) continue;
            const uint32_t q = s.t * SM::PC + s.piece;
            const uint32_t idx = index(q);
            CHECK(idx < SM::kImgTabs * SM::PC, "%s L=%d E=%d: p %u source index %u outside the image", name, L, E, p,
                  idx);
            CHECK(idx == want(s.t) * SM::PC + s.piece, "%s L=%d E=%d: p %u source index %u, table %u expected", name,
                  L, E, p, idx, want(s.t));
            if (s.real) {
                CHECK(at(q) == p, "%s L=%d E=%d: p %u -> q %u -> p %u", name, L, E, p, q, at(q));
                ++count[q];
            } else {
                CHECK(p % SM::SPC >= SM::PC, "%s L=%d E=%d: p %u is padding but piece %u is read", name, L, E, p,
                      p % SM::SPC);
            }
        }
    }
    for (uint32_t q = 0; q < pieces; ++q) {
        CHECK(count[q] == 1, "%s L=%d E=%d: piece %u produced %u times", name, L, E, q, count[q]);
        const uint32_t p = at(q);
        CHECK(p < N, "%s L=%d E=%d: piece %u at position %u of %u", name, L, E, q, p, N);
        const auto s = inv(p);
        CHECK(s.real && s.t * SM::PC + s.piece == q, "%s L=%d E=%d: q %u -> p %u -> q %u", name, L, E, q, p,
              s.t * SM::PC + s.piece);
    }
}

template <int L, int E>
void check_shape() {
    using SM = rs::EncodeStageMap<L, E>;
    constexpr uint32_t B0 = L >= 11 ? 1 : 0, IW = 7;
    const uint32_t waves = SM::n / SM::W;
    for (uint32_t wave = 0; wave < waves; ++wave) {
        // the layer order of a wave region: layers B0..IW-1, largest first
        std::vector<uint32_t> tabs;
        for (uint32_t b = B0; b < IW; ++b)
            for (uint32_t g = 0; g < (SM::W >> (b + 1)); ++g)
                tabs.push_back(SM::n - (SM::n >> b) + wave * (SM::W >> (b + 1)) + g);
        CHECK(tabs.size() == SM::kUp, "L=%d: %zu tables in the layer order, kUp %u", L, tabs.size(), SM::kUp);
        auto want = [&](uint32_t t) { return tabs[t]; };
        auto index = [&](uint32_t q) { return SM::priv_index(wave, q); };
        auto inv1 = [&](uint32_t p) {
            const auto s = SM::inv1(p);
            // the kernel's form: the layer mask first, then the table from the mask
            const uint32_t mask = SM::layer_mask(p / SM::SPC, SM::kSeq);
            const auto m = SM::inv1_mask(p, mask);
            CHECK(m.t == s.t && m.piece == s.piece && m.real == s.real, "L=%d E=%d: inv1_mask differs at %u", L, E, p);
            if (s.t < SM::kUp)
                CHECK(SM::priv_table_mask(wave, s.t, mask) == SM::priv_table(wave, s.t, SM::priv_layer(s.t)),
                      "L=%d E=%d wave %u: priv_table_mask of table %u", L, E, wave, s.t);
            return s;
        };
        auto at1 = [](uint32_t q) { return SM::at1(q); };
        check_region<SM>("phase 1", L, E, SM::kUp, SM::kPriv, inv1, at1, index, want);
        check_region<SM>("phase 3", L, E, SM::kP3, SM::kPriv, inv1, at1, index, want);
        if (B0) {
            auto want0 = [&](uint32_t t) { return wave * SM::kL0 + t; };  // layer 0: image tables 0 .. n/2
            check_region<SM>(
                "layer-0 turn", L, E, SM::kL0, SM::kPriv, [](uint32_t p) { return SM::inv0(p); },
                [](uint32_t q) { return SM::at0(q); }, [&](uint32_t q) { return SM::l0_index(wave, q); }, want0);
        }
    }
    if (SM::kShared) {
        // IFFT layers IW..L-1 of the IFFT image, then FFT layers FLO..L-1 of the FFT image
        std::vector<uint32_t> tabs;
        for (uint32_t b = IW; b < uint32_t(L); ++b)
            for (uint32_t g = 0; g < (SM::n >> (b + 1)); ++g) tabs.push_back(SM::n - (SM::n >> b) + g);
        CHECK(tabs.size() == SM::kShI, "L=%d: shared IFFT part %zu, kShI %u", L, tabs.size(), SM::kShI);
        for (uint32_t b = IW; b < uint32_t(L); ++b)  // (FLO = IW for these encodes)
            for (uint32_t g = 0; g < (SM::n >> (b + 1)); ++g) tabs.push_back(SM::n - (SM::n >> b) + g);
        CHECK(tabs.size() == SM::kShared, "L=%d: shared %zu, kShared %u", L, tabs.size(), SM::kShared);
        for (uint32_t q = 0; q < SM::kShared * SM::PC; ++q)
            CHECK(SM::shared_from_fft(q) == (q / SM::PC >= SM::kShI), "L=%d E=%d: image of shared piece %u", L, E, q);
        check_region<SM>(
            "shared", L, E, SM::kShared, SM::kShared, [](uint32_t p) { return SM::invS(p); },
            [](uint32_t q) { return SM::atS(q); }, [](uint32_t q) { return SM::shared_index(q); },
            [&](uint32_t t) { return tabs[t]; });
    }
    // sg / sg_inv over a whole layer-0 range, sq / sq_inv over every sequence length in use
    for (uint32_t g = 0; g < SM::n / 2; ++g)
        CHECK(SM::sg_inv(SM::sg(g)) == g && SM::sg(SM::sg_inv(g)) == g, "L=%d E=%d: sg at %u", L, E, g);
    for (uint32_t k = 1; k <= IW; ++k)
        for (uint32_t t = 0; t + 1 < (1u << k); ++t) {
            const uint32_t s = SM::sq(t, k);
            CHECK(s + 1 < (1u << k) && SM::layer_mask(s, k) == SM::layer_mask(t, k) && SM::sq_inv(s, k) == t,
                  "L=%d E=%d: sq(%u, %u) = %u", L, E, t, k, s);
        }
}

template <int E>
void check_format() {
    check_shape<7, E>();
    check_shape<8, E>();
    check_shape<9, E>();
    check_shape<10, E>();
    check_shape<11, E>();
}

}  // namespace

int main() {
    check_format<2>();
    check_format<4>();
    if (g_fail) {
        std::printf("stage map: %d checks failed\n", g_fail);
        return 1;
    }
    std::printf("stage map ok\n");
    return 0;
}
