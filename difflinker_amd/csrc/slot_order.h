// Slots of the pair loops (egnn_fc.hip, pair_phase): how many chunks a receiver's senders are cut into, which lane pair
// walks which (receiver, chunk), and how many steps a wave runs.  Plain C++ as well as HIP: tests/test_slot_order_host.py
// compiles this file with the host compiler and checks the map for every size.
#pragma once

#if defined(__HIPCC__)
#define DL_SLOT_HD __host__ __device__ __forceinline__
#else
#define DL_SLOT_HD inline
#endif

constexpr int SLOT_WAVES = 8;                         // waves of a workgroup
constexpr int NSLOT = 32 * SLOT_WAVES;                // lane pairs (c, c + 32) of the workgroup: one slot each

struct SlotPlan {
    int g, q;                                         // chunks per receiver, senders per chunk (= steps of the loop)
};
// nrec receivers share the 256 slots (all n_b atoms of the molecule, or this workgroup's part of them in a team)
DL_SLOT_HD SlotPlan slot_plan(int nrec, int nb) {
    SlotPlan sp;
    const int per = NSLOT / (nrec > 1 ? nrec : 1);
    sp.g = per < nb ? per : nb;
    sp.q = (nb + sp.g - 1) / sp.g;
    // ... and of the plans with that many steps the one with the FEWEST slots: a wave without slots skips the loop (8 linker atoms
    // as receivers of 50 senders: 25 instead of 32 slots each, 7 waves instead of 8; 36 atoms: 6 instead of 7, 7 waves) - a step
    // costs its energy per ACTIVE wave, and under the power cap energy is time (round 6)
    sp.g = (nb + sp.q - 1) / (sp.q > 1 ? sp.q : 1);
    // (one or two MORE steps where that takes fewer wave-steps still - 38 atoms: 6 waves x 8 instead of 8 x 7 - measured slower, +5 %:
    // the number of steps is the critical path; profiles/r06/ab_fewest_slots_plan.log)
    return sp;
}

// The last chunk of a receiver holds r = nb - (g - 1) q senders, 1 <= r <= q.  Where it is SHORT (g >= 2 and r < q) the
// slots are numbered with the nrec (g - 1) full chunks first, receiver-major, and the nrec short chunks behind them: the
// short slots fill whole waves at the end of the workgroup, and a wave that holds nothing else runs r steps and leaves -
// a step is paid per active wave (46 atoms: q, g, r = 10, 5, 6; waves 6 and 7 run 6 steps: 72 wave-steps instead of 80).
// Otherwise (r = q, or one chunk) slot = il g + c, receiver-major, and every active wave runs q steps.
// A slot still is one receiver and one contiguous sender range j0 .. j0 + jn - 1, and its partial sum keeps its place in
// LDS (row il g + c): only the lane that computes it differs, so no sum changes a bit.
struct SlotOrder {
    int g, q;
    int r;                                            // senders of a receiver's last chunk
    int first_short;                                  // short case: nrec (g - 1), the first short slot; otherwise -1
    int nslots;                                       // nrec g
};
DL_SLOT_HD SlotOrder slot_order(int nrec, int nb, bool receiver_major = false) {
    const SlotPlan pl = slot_plan(nrec, nb);
    SlotOrder so;
    so.g = pl.g;
    so.q = pl.q;
    so.r = nb - (pl.g - 1) * pl.q;
    so.nslots = nrec * pl.g;
    so.first_short = (!receiver_major && pl.g >= 2 && so.r < pl.q) ? nrec * (pl.g - 1) : -1;
    return so;
}

struct SlotLane {
    bool ok;                                          // the slot has a (receiver, chunk); the rest is zero otherwise
    int il, c;                                        // position of the receiver among the nrec, chunk
    int j0, jn;                                       // first sender, number of senders
};
// a / b for 0 <= a < 1024 and 1 <= b <= 256 without the integer-division sequence (some forty instructions per lane, twice per
// pass): (a + 0.5) / b is at least 0.5 / b >= 1.9e-3 away from every integer, and the rounding of the reciprocal and of the
// product moves it by less than 2e-4, so the truncation is exact
DL_SLOT_HD int slot_div(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return int((float(a) + 0.5f) * __builtin_amdgcn_rcpf(float(b)));
#else
    return int((float(a) + 0.5f) * (1.0f / float(b)));
#endif
}
DL_SLOT_HD SlotLane slot_lane(const SlotOrder& so, int nb, int slot) {
    SlotLane sl;
    sl.ok = slot < so.nslots;
    const bool gathered = so.first_short >= 0;
    const int d = gathered ? so.g - 1 : so.g;         // chunks per receiver among the slots numbered receiver-major
    int il = slot_div(slot, d);
    int c = slot - il * d;
    if (gathered && slot >= so.first_short) {
        il = slot - so.first_short;
        c = so.g - 1;
    }
    sl.il = sl.ok ? il : 0;
    sl.c = sl.ok ? c : 0;
    sl.j0 = sl.c * so.q;
    const int left = nb - sl.j0;
    sl.jn = sl.ok ? (so.q < left ? so.q : left) : 0;
    return sl;
}
// steps of wave w (slots 32 w .. 32 w + 31); wave-uniform.  0: the wave has no slot and skips the loop
DL_SLOT_HD int slot_wave_steps(const SlotOrder& so, int w) {
    if (32 * w >= so.nslots) return 0;
    return (so.first_short >= 0 && 32 * w >= so.first_short) ? so.r : so.q;
}
