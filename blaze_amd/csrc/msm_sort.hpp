// The three digit sorts and the unit lists as the sort stage (msm_sort_stage.hip msm_sort_stage()) calls them: included by the
// four sort files only.  Which one a task gets is plan_sort()'s decision (msm_engine.hpp SortPlan); the engine sees none of these.
#pragma once
#include "msm_engine.hpp"

namespace blz {

// The sort stages enqueue on C.sort_stream and fill C.B for the plan C.P; the scratch they share is the engine's.  Two-level LDS-privatised digit
// sort (msm_sort.hip): msm_sort_lds fills count[]; after the caller's scan msm_sort_lds_scatter fills entries[] from the intermediate described by `pass`
struct LdsSortPass {
    uint32_t slices = 0, nc = 0;           // fine-pass work items (upper bound), coarse bins
    int cl = 0;                            // log2 of the buckets per coarse bin
    const uint16_t* inter_fine = nullptr;  // u16 fine digits of the sort intermediate (second half of `inter`)
};
int msm_sort_lds(MsmEngine& E, const MsmStep& C, const void* d_scalars, uint32_t npts, int sbits, LdsSortPass& pass);
int msm_sort_lds_scatter(MsmEngine& E, const MsmStep& C, const LdsSortPass& pass);
// three-level, small-footprint digit sort built to run underneath another task's k_accumulate (msm_sort3.hip): fills count[] and
// entries[].  One family of kernels for plain plans and for window-table plans (P.table: shared bucket set, entries = point * W +
// window)
int msm_sort3(MsmEngine& E, const MsmStep& C, const void* d_scalars, uint32_t npts, int sbits);
// the whole sort stage of a small task (digits, bucket scan, entries, unit lists, stats) in one block (msm_sort_tiny.hip)
int msm_sort_tiny(MsmEngine& E, const MsmStep& C, const void* d_scalars, uint32_t npts, int sbits, uint32_t max_units);
int launch_fill_units(const MsmStep& C, uint32_t units);  // unit->bucket map + length-ordered unit list (at most `units` units)

}  // namespace blz
