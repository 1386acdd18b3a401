// The launch policy of a step's bf16 object work: the ONE place that reads DURF_OVERLAP_OBJECTS, DURF_OBJ_MSPLIT and
// DURF_OBJ_MIX and that compares a row count with DURF_OVERLAP_MIN_ROWS.  Both orchestrations (the Python-issued step through
// durf_step_policy, the one-call entry points through overlap_for) and the launchers ask it; no result depends on the answer.
#pragma once
#include <cstdlib>
#include <cstring>
#include "../../include/durf_hip.h"

namespace durf {

struct StepPolicy {
    bool side_fwd, side_bwd, side_dw;      // the object forward / backward / weight gradients on the side stream
    bool msplit;                           // W = 128 launches on compacted ray lists take the M-split kernels
    bool mix_enabled;                      // ... and may ride in the background MLP's persistent launches (on ONE stream: the caller's part)
    bool side() const { return side_fwd || side_bwd || side_dw; }
    unsigned bits() const {
        return (side_fwd ? DURF_POLICY_SIDE_FWD : 0u) | (side_bwd ? DURF_POLICY_SIDE_BWD : 0u) | (side_dw ? DURF_POLICY_SIDE_DW : 0u) |
               (msplit ? DURF_POLICY_MSPLIT : 0u) | (mix_enabled ? DURF_POLICY_MIX : 0u);
    }
};

// `rows`: sample rows per level.  DURF_OVERLAP_OBJECTS: unset / "auto" = "2" from DURF_OVERLAP_MIN_ROWS, else "0"; "1" the
// object forward on the side stream, "3" forward + backward, "2" forward + backward + weight gradients, anything else none.
// DURF_OBJ_MSPLIT=0 / DURF_OBJ_MIX=0: A/B switches.  Read per call (the tests toggle them); the host must not call setenv
// concurrently with a step.
inline StepPolicy step_policy(size_t rows) {
    const bool large = rows >= DURF_OVERLAP_MIN_ROWS;
    const char* e = getenv("DURF_OVERLAP_OBJECTS");
    if (e == nullptr || !strcmp(e, "auto")) e = large ? "2" : "0";
    const char* ms = getenv("DURF_OBJ_MSPLIT");
    const char* mx = getenv("DURF_OBJ_MIX");
    StepPolicy p;
    p.side_dw = !strcmp(e, "2");
    p.side_bwd = p.side_dw || !strcmp(e, "3");
    p.side_fwd = p.side_bwd || !strcmp(e, "1");
    p.msplit = !large && !(ms && ms[0] == '0');
    p.mix_enabled = p.msplit && !(mx && mx[0] == '0');
    return p;
}

}  // namespace durf
