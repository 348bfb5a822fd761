// ctg_exec_state.h -- the opaque handles of include/ctg_hip.h as seen by the
// host-side translation units of the library: ctg_runtime.hip, ctg_collective.hip,
// ctg_lds_host.hip, ctg_range.hip and, through
// ctg_result_host.h, the sources that read the result tensor (ctg_sample.hip,
// ctg_reduce.hip, ctg_rdm.hip, ctg_pauli.hip, ctg_pauli_apply.hip, ctg_op_apply.hip).
// Not installed; not part of the ABI.
#pragma once

#include <string>
#include <vector>

#include "../../include/ctg_hip.h"
#include "ctg_common.h"
#include "ctg_lds.h"

struct ctg_plan {
    int dtype = 0;
    int64_t n_inputs = 0;
    std::vector<int64_t> input_sizes, input_offsets;
    int64_t inputs_elems = 0, arena_elems = 0, result_elems = 0;
    int64_t n_steps = 0;
    std::vector<int64_t> steps;
    std::vector<int64_t> tables;
    int64_t n_sliced = 0;
    std::vector<int64_t> slice_sizes, slice_fixed, slice_strides;
    std::vector<int64_t> slice_group;   // [n_sliced] 1: a group index (ctg_plan_desc.slice_group)
    bool has_groups = false;            // some step is shared by the slices of a group (word 42 = 2)
    int64_t nslices = 1;
    // per-leaf maximum slice offset (for bounds validation)
    std::vector<int64_t> max_soff;
};

struct ctg_exec {
    const ctg_plan* plan = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    char* d_inputs = nullptr;
    char* d_arena = nullptr;
    char* d_result = nullptr;
    bool owns_result = false;
    // float / complex64 results of a sliced tree: the running sum of the slices in double precision (same
    // element offsets as the result, which always holds this sum rounded once); null otherwise
    char* d_wide = nullptr;
    // single-precision trees: [n_inputs offsets | n_inputs sizes] of the inputs space, and {2^S, S log10(2), (int) S}
    // -- the power of two taken out of the inputs at upload (prescale_inputs_kernel); null otherwise
    int64_t* d_in_tab = nullptr;
    double* d_inscale = nullptr;
    int64_t* d_tables = nullptr;
    int64_t* d_misc = nullptr;  // [state(2) | zero(1) | soff(n_leaves) | sizes | fixed | strides]
    int64_t* d_state = nullptr;
    int64_t* d_zero = nullptr;
    int64_t* d_soff = nullptr;
    void* d_scratch = nullptr;
    ctg::SliceMeta meta{};
    std::vector<ctg::StepArgs> args;  // resolved per step
    std::vector<ctg::StemArgs> stem_args;  // KIND_STEM2 steps (fused stem pairs)
    int stem_bf16x3 = 1;                   // ctg_exec_set_stem_arithmetic (default since round 4: bf16 x 3)
    // (round 6) 2: the stem kernels multiply with two fp16 limbs and three products (ctg_stem_h2.hip: stem2h_kernel)
    // where they took three bf16 limbs and six; stem_bf16x3 stays 1 then (the bf16-pipe kernels are on)
    int stem_arith = 2;
    // [3 banks][n_steps][batch][kMaxSub]: largest |component| recorded by step s in slice z of a launch sequence | of step s's
    // operand A | B (max-abs pass): smax_slot().  A slice-invariant step records into z = 0.
    // A producer only raises its record, so the prologue in front of it sets the record to zero: the one before a
    // slice resets the per-slice steps' and the group-shared steps', the one before the slice-invariant steps of a
    // new upload every record -- what an executor returns never depends on what it ran before.
    float* d_stem_max = nullptr;
    // [3 masks][n_steps][batch][kMaxSub]: the records of bank 0 that a prologue sets to zero -- 0: before every
    // step of a slice, 1: before a slice that reuses its group's shared steps, 2: before the slice-invariant steps
    int32_t* d_smax_zero = nullptr;
    float* smax_slot(int bank, int64_t s, int64_t z) const {
        return d_stem_max + (((int64_t)bank * plan_steps + s) * (batch > 1 ? batch : 1) + z) * ctg::kMaxSub;
    }
    // `meta` for a prologue that resets the records of mask `which` (meta itself: mask 0)
    ctg::SliceMeta meta_resetting(int which) const {
        ctg::SliceMeta m = meta;
        if (m.smax) m.smax_zero = d_smax_zero + (int64_t)which * m.n_smax;
        return m;
    }
    int64_t plan_steps = 0;                // (= plan->n_steps, for smax_slot)
    std::vector<char> rec_wanted;          // the record of step s's largest |component| has a reader (build_hints)
    std::vector<char> wave_member;         // step s is launched inside a wave-front group (it never records its maximum)
    std::vector<char> stem_paired_ran;     // step s last ran a kernel with paired 16-byte stores (ctg_exec_step_paired_stores)
    std::vector<char> stem_h2_ran;         // step s last ran in the fp16 x 2 arithmetic (its record is valid)
    std::vector<ctg::MfmaHints> hints;  // per step kernel hints (MFMA steps)
    // the same for launches that carry several slices (batch > 1): wider column tiles
    // where one slice alone would not fill the chip; same k-splits, same kernels otherwise
    std::vector<ctg::MfmaHints> hints_b;
    uint16_t* d_ord_b = nullptr;
    char* d_lane_b = nullptr;
    uint16_t* d_ord = nullptr;     // order tables of all MFMA steps
    char* d_lane = nullptr;        // lane-constant tables of the fast tiled steps
    // slice batching: up to `batch` slices of a run share every launch (gridDim.y);
    // the arena holds `batch` replicas of itself, d_soff `batch` rows of leaf offsets
    int batch = 1;
    // slice groups in batched launches: slices per group (0: the plan has no groups or slices go one by
    // one), the ids of the slices of the launch at hand (device, `batch` entries)
    int group_d = 0;
    int64_t* d_batch_ids = nullptr;
    int64_t* h_ids = nullptr;      // pinned staging of the ids of batched group launches (run_grouped)
    size_t h_ids_cap = 0;
    hipEvent_t ev_ids = nullptr;   // ... recorded after the last copy out of it
    int batch_nominal = 1;         // min(64, nslices, 8 GiB / arena): what the k-splits are chosen for
    int64_t scratch_total = 0;     // bytes of d_scratch (64 MiB x up to 8 for batching executors)
    // the launch list of one slice: steps that launch alone (cls < 0) and wave-front
    // groups -- n independent small steps of one kernel shape sharing a launch (cls 0:
    // thread-per-output items, 1 + key: tiled fast-kernel items, starting at item0; -2 LDS-resident subtrees;
    // -3 consecutive accumulate steps)
    struct Issue {
        int64_t step;
        int cls;
        int32_t item0, n;
        uint32_t blocks;
        bool shared = false;   // steps the slices of a group share (all members of a wave-front group alike)
    };
    std::vector<Issue> issue;
    std::vector<Issue> issue_reuse;   // ... of a slice that finds the shared steps of its group done
    // LDS-resident subtrees (round 6; ctg_lds_host.hip / ctg_lds_run.hip): per step the packed component that
    // runs it (-1: none, the step launches as usual); components sorted [group-shared..., per-slice...]
    std::vector<int32_t> lds_comp_of;
    int lds_first[2] = {0, 0}, lds_count[2] = {0, 0}, lds_bytes[2] = {0, 0};   // [0] group-shared, [1] per slice
    std::vector<std::vector<ctg::LdsForm>> lds_forms;   // per packed component, in record order (ctg_exec_lds_form)
    ctg::LdsCompDev* d_lds_comps = nullptr;
    char* d_lds_blob = nullptr;
    ctg::ValuGroupItem* d_group_items = nullptr;
    // (ABI 8) runs of consecutive accumulate steps sharing one launch (cls -3 of Issue: accum_group_kernel), and
    // which steps are members of such a run
    ctg::AccumGroupItem* d_accum_items = nullptr;
    std::vector<char> accum_member;
    ctg::FastGroupItem* d_fast_items = nullptr;
    std::vector<hipEvent_t> events;
    // slice graph: the launch sequence of one slice captured once and replayed,
    // the slice id advancing on the device (prologue kernel)
    hipStream_t gstream = nullptr;
    hipGraphExec_t gexec = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    bool warm = false;
    bool soff_static = false;      // unsliced tree: the (all-zero) leaf offsets are in place
    bool graph_off = false;
    // strip_exponent state
    int strip = 0, check_zero = 0;
    double* d_fac = nullptr;        // [n_steps + 1] max|.| per pair step; last = constant 1.0
    int32_t* d_counted = nullptr;   // [n_steps] 1 for pair steps; 2: the zero test alone (zero_probe_step)
    int32_t* d_fac_zero = nullptr;  // [n_steps] 1 for per-slice pair steps
    // the accumulate step of a plan without a pair step (a one-input tree), -1 otherwise: nothing is normalised there,
    // but check_zero still looks for a zero slice -- a max-abs pass over what the step adds fills its slot of d_fac
    int64_t zero_probe_step = -1;
    // slice-invariant steps: executed once per upload / option change
    std::vector<char> invariant;
    bool invariants_ready = false;
    // steps shared by the slices of a group: executed when the group key changes
    std::vector<char> grouped;
    int64_t group_key = -1;
    ctg::StripState* d_strip = nullptr;
    int64_t root_step = -1;
    // (ABI 9) statistics of / draws from the result tensor (ctg_sample.hip): the per-block sums and their prefix
    // sums, the uniforms and outputs of one chunk of draws -- allocated by the first call, grown on demand
    void* d_sample_blocks = nullptr;
    void* d_sample_io = nullptr;
    int64_t sample_blocks_bytes = 0, sample_io_bytes = 0;
    // what the last statistics / sample call found ({sum p, sum p^2, max p, bits of argmax}) and the device time of its
    // passes 1 and 2 (events on the executor's stream): ctg_exec_sample_info
    double sample_last[4] = {0, 0, 0, 0};
    float sample_pass_ms[2] = {0, 0};
    bool sample_last_valid = false;
    hipEvent_t sample_ev[3] = {nullptr, nullptr, nullptr};
    // (ABI 10) the range audit (ctg_range.hip, ctg_exec_range_audit): [rows (n_inputs + n_steps) x CTG_RANGE_WORDS |
    // sums of squares | the pass's per-workgroup rows] -- allocated by the first call, grown on demand
    void* d_range = nullptr;
    int64_t range_bytes = 0;
    // top-k and marginals of the result tensor (ctg_reduce.hip): digit counts, block counts and their scans, the
    // compact key list and the k records / the output and the partial sums of a slab -- allocated by the first call,
    // grown on demand
    void* d_reduce = nullptr;
    int64_t reduce_bytes = 0;
};


// element size in bytes by CTG_* dtype code
inline int64_t ctg_item_size(int dtype) {
    static const int64_t k[4] = {4, 8, 8, 16};
    return k[dtype];
}

// records `msg` as the calling thread's ctg_last_error() (ctg_runtime.hip)
extern "C" __attribute__((visibility("hidden"))) void ctg_set_error_(const char* msg);

namespace ctg {
// (ctg_kernels_valu.hip) largest |re|, |im| of n complex64 values as a float; *out zeroed by the caller
// (nz slices from z on: the record (kMaxSub floats, zeroed by the caller) at out + i * out_zs for slice z + i)
hipError_t launch_maxabs_f32(const void* base, const int64_t* soff, int64_t z, int64_t zs, int64_t zstride, int64_t n,
                             float* out, hipStream_t stream, int nz = 1, int out_zs = 0);
}

namespace ctg {
// (ctg_range.hip) exponent histogram, zero count and sum of squares of n contiguous fp32 components at x:
// row <- {1, n, zeros, 0, hist[256]} and *sumsq (device memory), through `partials` (range_partial_bytes(blocks)
// bytes of device memory, blocks >= range_blocks(n)).  Reads [x, x + n) only; the caller checks that range.
constexpr int64_t kRangeMaxBlocks = 2048;              // workgroups of the pass (a workgroup takes several chunks)
constexpr int64_t kRangeMaxComponents = 1ll << 40;     // (a workgroup's 32-bit counts hold its share)
int64_t range_blocks(int64_t n);
int64_t range_partial_bytes(int64_t blocks);
hipError_t launch_range_hist(const void* x, int64_t n, void* partials, int64_t blocks, int64_t* row, double* sumsq,
                             hipStream_t stream);
}

namespace ctg {
// (ctg_reduce.hip) What the host decides about a marginal -- or a reduced density matrix (ctg_rdm.hip), which splits the
// axes the same way -- before anything is launched: size-1 axes dropped, adjacent axes of equal keep status merged;
// the route; the keep bitmask of the power-of-two route; extents and strides of the kept / dropped axes otherwise.
constexpr int kMargMaxAxes = 32;                 // merged axes of one keep status (extents >= 2: 2^31 elements each way)
constexpr int64_t kReduceMaxElems = 1ll << 40;   // (a workgroup's 32-bit counts hold its share of a digit pass)
struct MargAxes {
    int nk, nd;
    int64_t kext[kMargMaxAxes], kstr[kMargMaxAxes], dext[kMargMaxAxes], dstr[kMargMaxAxes];
};
struct MarginalPlan {
    int64_t n = 1, m = 1, rc = 1;
    bool fast = false;
    int64_t mask = 0;
    MargAxes ax{};
};
// CTG_OK, or CTG_E_INVALID with *why set
__attribute__((visibility("hidden"))) int marginal_plan(int64_t rank, const int64_t* extents, const int32_t* keep,
                                                        int64_t result_elems, MarginalPlan* out, const char** why);
// the executor's scratch of ctg_reduce.hip / ctg_rdm.hip / ctg_pauli.hip / ctg_pauli_apply.hip / ctg_op_apply.hip (d_reduce, laid
// out by Carve of ctg_result_host.h), at least `want` bytes; the stream must be idle
// (the statistics call synchronised it).  CTG_OK, CTG_E_NOMEM or CTG_E_HIP with the error set.
__attribute__((visibility("hidden"))) int reduce_reserve(ctg_exec* e, int64_t want);
}

// LDS-resident subtrees (ctg_lds_host.hip): descriptor validation (host only) and per-executor packing
__attribute__((visibility("hidden"))) int ctg_lds_validate(const ctg_plan* p);
__attribute__((visibility("hidden"))) int ctg_lds_build(ctg_exec* e);
// the host half of ctg_lds_build on its own -- forms and packing from the plan alone, nothing uploaded (-> a digest)
__attribute__((visibility("hidden"))) int64_t ctg_lds_host_reads(const ctg_plan* p);
// (ctg_runtime.hip) every host function executor creation runs over a validated plan's tables, without a device
extern "C" __attribute__((visibility("hidden"))) int64_t ctg_plan_host_reads_(const ctg_plan* p);
