// Compile-time plan of the column kernel (rs_mono.hip): which row bit sits in which
// register, lane or wave bit before every op of a transform, and the ops themselves
// (butterfly layers, register/lane transposes, LDS remaps).  Plain constexpr C++ (no
// device headers): the kernel and a host test (tests/split_plan_check.cpp) compile the
// same text.
#pragma once

namespace rs {
namespace {

// ---------------------------------------------------------------------------
// compile-time plan

struct Map {
    int reg[3];   // row bit held by register-index bit s
    int lane[6];  // row bit held by lane bit j
    int wave[4];  // row bit held by wave bit k
};
enum : int { kOpLayer = 1, kOpXpose = 2, kOpRemap = 3 };
struct Op {
    int kind, bit, rs, ls;  // layer on `bit` (register bit rs) / swap register bit rs with lane bit ls
};
constexpr int kMaxOps = 64;
struct Seq {
    int count = 0;
    Op ops[kMaxOps] = {};
    Map maps[kMaxOps + 1] = {};  // maps[i]: placement before op i; maps[count]: final
};

constexpr int find_reg(const Map &m, int LR, int x) {
    for (int s = 0; s < LR; ++s)
        if (m.reg[s] == x) return s;
    return -1;
}
constexpr int find_lane(const Map &m, int x) {
    for (int j = 0; j < 6; ++j)
        if (m.lane[j] == x) return j;
    return -1;
}
constexpr int next_use(const int *bits, int nb, int from, int x) {
    for (int t = from; t < nb; ++t)
        if (bits[t] == x) return t;
    return 1 << 20;
}
constexpr void push(Seq &s, Op op, const Map &after) {
    s.ops[s.count] = op;
    ++s.count;
    s.maps[s.count] = after;
}

// Butterfly layers on `bits` in order; a bit not in a register is swapped in
// from its lane bit, evicting the register bit used furthest in the future.
constexpr void layers(Seq &s, Map &m, int LR, const int *bits, int nb) {
    for (int t = 0; t < nb; ++t) {
        const int x = bits[t];
        int rs = find_reg(m, LR, x);
        if (rs < 0) {
            const int j = find_lane(m, x);
            int far = -1;
            for (int q = 0; q < LR; ++q) {
                const int u = next_use(bits, nb, t + 1, m.reg[q]);
                if (u > far) far = u, rs = q;
            }
            const int tmp = m.reg[rs];
            m.reg[rs] = m.lane[j];
            m.lane[j] = tmp;
            push(s, Op{kOpXpose, x, rs, j}, m);
        }
        push(s, Op{kOpLayer, x, rs, 0}, m);
    }
}

// Placement of a segment: in-wave bits [lo, lo + IW), wave bits the rest.
// Registers take the first bits of `order`; lane bits the next ones, cheapest
// transposes (permlane swaps: lane bits 5, 4; DPP: 0, 1, 3; two DPP moves: 2) first.
// pin >= 0 (pair plans, Plan): bit `pin` sits on lane bit 0 whatever the order says, and
// the in-wave bits are `pin` and [lo, lo + IW - 1).
constexpr Map seg_map(int L, int LR, int lo, const int *order, int no, int pin = -1) {
    const int IW = LR + 6, hi = lo + IW - (pin >= 0 ? 1 : 0);
    int pri[16] = {}, np = 0;
    for (int t = 0; t < no; ++t) {
        const int x = order[t];
        bool seen = x < lo || x >= hi;
        for (int q = 0; q < np; ++q) seen = seen || pri[q] == x;
        if (!seen) pri[np++] = x;
    }
    for (int x = lo; x < hi; ++x) {
        bool seen = false;
        for (int q = 0; q < np; ++q) seen = seen || pri[q] == x;
        if (!seen) pri[np++] = x;
    }
    const int pref[6] = {5, 4, 0, 1, 3, 2};
    Map m{};
    for (int s = 0; s < 3; ++s) m.reg[s] = s < LR ? pri[s] : -1;
    int q = LR;
    for (int j = 0; j < 6; ++j) {
        if (pin >= 0 && pref[j] == 0) m.lane[0] = pin;
        else m.lane[pref[j]] = pri[q++];
    }
    int k = 0;
    for (int x = 0; x < L; ++x)
        if (x != pin && (x < lo || x >= hi)) m.wave[k++] = x;
    for (; k < 4; ++k) m.wave[k] = -1;
    return m;
}

// SPLIT (decodes whose restored rows lie in one half of the 2^L work rows):
// the top row bit L-1 stays a wave bit throughout, so each half is a 2^(L-1)
// row transform of its own waves; the IFFT stops below layer L-1, the top
// layers of both transforms and the formal derivative's cross-half term run
// in one exchange (split_top), and only the half holding restored rows runs
// the rest of the FFT.
// SP bit 1 (FLOW, decodes): the FFT leaves the top placement after layer IW
// instead of WB, so its layers IW-1..0 run with the low bits in-wave -- each
// wave then holds 2^IW consecutive rows, the waves without restored rows stop
// there, and those layers reuse the IFFT's phase-1 tables
// SP bit 2 (PAIR, the split encode k_mono_split): a register holds one byte plane of a
// PAIR row (rows 2q, 2q + 1) and the plane is lane bit 0, in every segment.  Bit 0 of
// the plan's row index is that plane, a pseudo row bit that is pinned (seg_map's pin)
// and never gets a layer or a transpose; bits 1..L-1 are the rows' own, so every map
// of the plan, the LDS plane's index and the tables' slots read as they do elsewhere.
// The rows' layer 0 runs inside a word, outside the sequences (split_layer0).  The top
// segment's in-wave bits: the plane and the top IW - 1 row bits
template <int L, int LR, int SP = 0>
struct Plan {
    static constexpr bool SPLIT = (SP & 1) != 0, FLOW = (SP & 2) != 0, PAIR = (SP & 4) != 0;
    static_assert(!PAIR || (!SPLIT && FLOW && L > LR + 6), "pair plan: the flow plan with wave bits");
    static constexpr int LOW = PAIR ? 1 : 0;    // lowest row bit that gets a layer
    static constexpr int PIN = PAIR ? 0 : -1;  // seg_map's pinned bit
    static constexpr int IW = LR + 6, WB = L - IW - (SPLIT ? 1 : 0), R = 1 << LR;
    static_assert(WB >= 0 && L - IW <= 4, "column kernel: 6 lane bits + LR register bits + up to 4 wave bits");
    static_assert(!SPLIT || WB >= 1, "split plan: at least one wave bit below the top bit");
    static constexpr int TOP = SPLIT ? L - 1 : L;  // layers [0, TOP) run in the sequences
    // lowest FFT layer of the top placement (the FFT's low segment: layers FLO-1..0)
    static constexpr int FLO = FLOW && WB > 0 ? IW : WB;

    static constexpr Seq make_ifft() {
        Seq s{};
        int bits[16] = {}, order[32] = {}, no = 0;
        if (WB == 0 && !SPLIT) {
            for (int x = 0; x < L; ++x) order[no++] = x;
            for (int x = L - 1; x >= 0; --x) order[no++] = x;
            Map m = seg_map(L, LR, 0, order, no);
            s.maps[0] = m;
            for (int x = 0; x < L; ++x) bits[x] = x;
            layers(s, m, LR, bits, L);
            return s;
        }
        // segment A: IFFT layers 0..IW-1 with the low bits in-wave
        for (int x = LOW; x < IW; ++x) order[no++] = x, bits[x - LOW] = x;
        Map m = seg_map(L, LR, LOW, order, no, PIN);
        s.maps[0] = m;
        layers(s, m, LR, bits, IW - LOW);
        // segment B: the top IW bits (below bit L-1 when SPLIT) in-wave: IFFT
        // layers IW..TOP-1 (then FFT TOP-1..WB)
        no = 0;
        for (int x = IW; x < TOP; ++x) order[no++] = x;
        for (int x = TOP - 1; x >= WB; --x) order[no++] = x;
        m = seg_map(L, LR, WB + LOW, order, no, PIN);
        push(s, Op{kOpRemap, -1, 0, 0}, m);
        for (int x = IW; x < TOP; ++x) bits[x - IW] = x;
        layers(s, m, LR, bits, TOP - IW);
        return s;
    }
    static constexpr Seq ifft = make_ifft();

    static constexpr Seq make_fft() {
        Seq s{};
        int bits[16] = {}, order[16] = {}, no = 0;
        Map m = ifft.maps[ifft.count];
        s.maps[0] = m;
        const int stop = FLO;  // FFT layers TOP-1..stop in the IFFT's final placement
        for (int x = TOP - 1; x >= stop; --x) bits[TOP - 1 - x] = x;
        layers(s, m, LR, bits, TOP - stop);
        if (WB == 0) return s;
        // segment C: the low IW bits in-wave again, FFT layers FLO-1..0
        for (int x = FLO - 1; x >= LOW; --x) order[no++] = x;
        m = seg_map(L, LR, LOW, order, no, PIN);
        push(s, Op{kOpRemap, -1, 0, 0}, m);
        for (int x = FLO - 1; x >= LOW; --x) bits[FLO - 1 - x] = x;
        layers(s, m, LR, bits, FLO - LOW);
        return s;
    }
    static constexpr Seq fft = make_fft();
};

template <int L, int LR, bool FFT, int SPLIT = 0>
struct SeqOf {
    static constexpr const Seq &v = FFT ? Plan<L, LR, SPLIT>::fft : Plan<L, LR, SPLIT>::ifft;
};

constexpr int layer_ordinal(const Seq &s, int i) {
    int k = 0;
    for (int q = 0; q < i; ++q) k += s.ops[q].kind == kOpLayer;
    return k;
}

}  // namespace
}  // namespace rs
