// What an mcl_context caches about the factors between its entry points, and what each cached by-product is computed from.
// Host code only (no HIP header).  An entry point says in ONE call what it is about to change - changed(IN_C | IN_ADMM(2)) -
// and the table below decides which by-products fall; the launch site that produced one says made(BP_...).  Nothing else
// writes a validity bit.
#pragma once
#include <cstdint>

// ---- the inputs a by-product can be computed from ---------------------------------------------------------------------
enum : uint32_t {
    IN_X = 1u << 0,          // the data matrices (mcl_set_problem: with them every shape)
    IN_A = 1u << 1,          // the factor of mode 0 / 1 / 2: IN_FACTOR(m)
    IN_B = 1u << 2,
    IN_C = 1u << 3,
    IN_ADMM0 = 1u << 4,      // the auxiliary and dual variables of mode m: IN_ADMM(m) (what a mode's diagnostics table reflects
                             // besides its factor)
    IN_PEN0 = 1u << 7,       // the penalty list of mode m: IN_PEN(m)
    IN_OPTIONS = 1u << 10,   // mcl_options
    IN_WORKSPACE = 1u << 11, // the workspace installation: every by-product lives in it
    IN_COUNT = 12
};
constexpr uint32_t IN_FACTOR(int m) { return IN_A << m; }
constexpr uint32_t IN_ADMM(int m) { return IN_ADMM0 << m; }
constexpr uint32_t IN_PEN(int m) { return IN_PEN0 << m; }
// all the state an outer iteration moves (mcl_set_factors: "the caller wrote the tensors"; a gated run that stopped early)
constexpr uint32_t IN_ALL_STATE = IN_A | IN_B | IN_C | IN_ADMM(0) | IN_ADMM(1) | IN_ADMM(2);

// ---- the by-products ----------------------------------------------------------------------------------------------------
enum Byproduct : int {
    BP_XC,         // XC (XC64) = X C, cached between the A-phase and the next B-phase
    BP_CTC,        // CtC / CtC64 = C^T C - while ctc_parts > 0 still as that many partial blocks in CtCpart
    BP_CFRAG,      // Cfrag: C in MFMA-fragment order (one image for the X C kernels and the sweep)
    BP_MPART,      // the sweep's Mpart / part_btb: per-bseg X^T B and B^T B
    BP_GRPART,     // the sweep's GRpart: per-bseg a-weighted [G | R]
    BP_E1,         // e1 / rhsA / BtB of the A-phase: the loss without a pass over X (e1_from_raw_gram: what BtB holds)
    BP_B_SYSTEMS,  // rhoB / LinvB already hold the systems of the coming B-phase (built by the fused A-phase finish)
    BP_A64,        // rhsA64 / Q64 / LinvA64: fp64 copies of the systems an un-fused A-phase finish built last
    BP_XSQ,        // x_sq = ||X||^2
    BP_DIAG0,      // the diagnostics table of mode m, diag_rows[m] rows of it: BP_DIAG(m)
    BP_DIAG1,
    BP_DIAG2,
    BP_COUNT
};
constexpr Byproduct BP_DIAG(int m) { return Byproduct(BP_DIAG0 + m); }

// ---- THE TABLE: what every by-product is computed from --------------------------------------------------------------------
constexpr uint32_t BP_DEPENDS_ON[BP_COUNT] = {
    /* BP_XC        */ IN_X | IN_C | IN_WORKSPACE,
    /* BP_CTC       */ IN_C | IN_WORKSPACE,
    /* BP_CFRAG     */ IN_C | IN_WORKSPACE,
    /* BP_MPART     */ IN_X | IN_B | IN_WORKSPACE,
    /* BP_GRPART    */ IN_X | IN_B | IN_A | IN_WORKSPACE,
    // (the kernel that leaves e1 also leaves the table of mode 0, penalty columns included)
    /* BP_E1        */ IN_X | IN_A | IN_B | IN_C | IN_PEN(0) | IN_WORKSPACE,
    // the systems C^T C o a_i a_i^T + (n rho_i + l2) I of the B-phase: no B in them
    /* BP_B_SYSTEMS */ IN_A | IN_C | IN_PEN(1) | IN_OPTIONS | IN_WORKSPACE,
    // the systems of an A-phase IN PROGRESS: built by mcl_A_factor / the un-fused finish from X, B and C, they stand while the
    // steps of that phase move A (mcl_A_solve .. mcl_A_end); a finish that runs the inner loop itself - and with it rewrites
    // the ADMM variables of mode 0 - starts from systems of its own
    /* BP_A64       */ IN_X | IN_B | IN_C | IN_ADMM(0) | IN_WORKSPACE,
    /* BP_XSQ       */ IN_X | IN_WORKSPACE,
    /* BP_DIAG0     */ IN_A | IN_ADMM(0) | IN_PEN(0) | IN_WORKSPACE,
    /* BP_DIAG1     */ IN_B | IN_ADMM(1) | IN_PEN(1) | IN_WORKSPACE,
    /* BP_DIAG2     */ IN_C | IN_ADMM(2) | IN_PEN(2) | IN_WORKSPACE,
};

// the by-products (bit p = by-product p) whose dependency set meets `inputs`
constexpr uint32_t bp_dependents(uint32_t inputs) {
    uint32_t m = 0;
    for (int p = 0; p < BP_COUNT; ++p)
        if (BP_DEPENDS_ON[p] & inputs) m |= 1u << p;
    return m;
}

namespace bp_checks {
constexpr bool every_byproduct_has_an_input() {
    for (int p = 0; p < BP_COUNT; ++p)
        if (BP_DEPENDS_ON[p] == 0 || (BP_DEPENDS_ON[p] >> IN_COUNT) != 0) return false;
    return true;
}
constexpr bool every_input_invalidates_something() {
    for (int i = 0; i < IN_COUNT; ++i)
        if (bp_dependents(1u << i) == 0) return false;
    return true;
}
static_assert(every_byproduct_has_an_input(), "a by-product that depends on nothing (or on an unknown input) can never fall");
static_assert(every_input_invalidates_something(), "an input nothing depends on: a changed() that names it does nothing");
// GRpart is Mpart's a-weighted twin out of the same sweep: the C-phase reduction takes both or neither
static_assert((BP_DEPENDS_ON[BP_GRPART] & BP_DEPENDS_ON[BP_MPART]) == BP_DEPENDS_ON[BP_MPART], "GRpart must fall with Mpart");
static_assert(BP_COUNT <= 32 && IN_COUNT <= 32, "the bits are one word");
}  // namespace bp_checks

// ---- the context's record -------------------------------------------------------------------------------------------------
struct Byproducts {
    // Values that mean something only while their by-product stands; the launch site that produced the by-product writes
    // them (BEFORE its caller says made()), and they are reset when it falls - so changed() comes before the launches of an
    // entry point, never after.
    int ctc_parts = 0;              // BP_CTC: > 0: as that many partial blocks in CtCpart, not yet folded (k_C_finish_multi)
    bool e1_from_raw_gram = false;  // BP_E1: the BtB buffer holds B_i^T B_i (true) or Q_i = B_i^T B_i o C^T C (false)
    int diag_rows[3] = {0, 0, 0};   // BP_DIAG(m): rows written in diagA_row / diagB_tile / diagC_tile

    bool has(Byproduct p) const { return (valid >> p) & 1u; }
    void made(Byproduct p) { valid |= 1u << p; }
    // the named inputs are about to change (or have just been replaced): everything computed from any of them falls
    void changed(uint32_t inputs) { drop(bp_dependents(inputs)); }
    // ONE by-product falls though no input moved: its buffers were given to something else, or it is used up by its consumer
    void dropped(Byproduct p) { drop(1u << p); }

   private:
    uint32_t valid = 0;
    void drop(uint32_t mask) {
        valid &= ~mask;
        if (mask >> BP_CTC & 1u) ctc_parts = 0;
        if (mask >> BP_E1 & 1u) e1_from_raw_gram = false;
        for (int m = 0; m < 3; ++m)
            if (mask >> BP_DIAG(m) & 1u) diag_rows[m] = 0;
    }
};
