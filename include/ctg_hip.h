/* ctg_hip.h -- C ABI of the MI355X-native contraction-tree executor.
 *
 * This is the drop-in boundary for the execution path of jcmgray/cotengra
 * (SURVEY.md section 8b).  cotengra itself is pure Python and has no FFI; the
 * slot this library fills is the one the reference gives to a whole-tree
 * native backend, `CuQuantumContractor` (reference cotengra/contract.py:840-922,
 * selected in `make_contractor`, contract.py:986-992): built once from a tree,
 * called with the input arrays, returns the contracted output.  Each entry
 * point below cites the reference behaviour it replaces.
 *
 * Conventions: every function returns 0 on success and a negative CTG_E_*
 * code on failure; `ctg_last_error()` returns a thread-local message for the
 * last failure.  Handles are opaque.  Host buffers are borrowed for the
 * duration of a call only and never written unless documented (the reference
 * never mutates its inputs: contract.py:779-807 only drops references).  All
 * device work is enqueued on the `stream` given at exec creation (a
 * `hipStream_t` passed as `void*`; NULL = the default stream) and is
 * asynchronous unless documented otherwise.  A `ctg_exec` is confined to one
 * host thread at a time (one per GPU); plans are immutable and shareable.
 *
 * No torch / numpy / Python types appear anywhere in this interface.
 */
#ifndef CTG_HIP_H
#define CTG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTG_ABI_VERSION 10

/* element types of the tensors (reference tests cover all four:
 * tests/test_compute.py:102-115) */
enum { CTG_F32 = 0, CTG_F64 = 1, CTG_C64 = 2, CTG_C128 = 3 };

enum {
    CTG_OK = 0,
    CTG_E_INVALID = -1, /* malformed plan / argument (ValueError in the reference) */
    CTG_E_HIP = -2,     /* a HIP runtime call failed */
    CTG_E_NOMEM = -3,   /* device allocation failed */
    CTG_E_BOUNDS = -4,  /* plan addresses outside a declared buffer */
    CTG_E_COMM = -5,    /* RCCL missing, or a collective call failed */
    CTG_E_NORM = -6     /* (ABI 9) nothing to draw from: the result tensor's sum of |x|^2 is zero or not finite */
};

#define CTG_STEP_WORDS 48

/* Flat description of a compiled plan (produced by cotengra_amd/plan.py).
 * It encodes what the reference keeps as the op list of
 * `extract_contractions` (contract.py:573-651) plus the per-step index
 * classification of `_parse_eq_to_batch_matmul` (contract.py:168-329), lowered
 * to offset tables; and the slice bookkeeping of `SliceInfo` /
 * `get_slice_strides` / `slice_key` (core.py:99-122, 3775-3800).
 *
 * Step kinds (word 0 of a step record): 0 single-term einsum (contract.py:62-119,
 * 332-361), 1 pairwise contraction (contract.py:364-411), 2 accumulate the slice
 * into the result (core.py:3842-3876), and -- ABI 3 -- 3: TWO consecutive pairwise
 * contractions of a stem executed as one launch whose intermediate never exists in
 * memory (two turns of the loop contract.py:788-832; complex64 only).  A kind-3
 * record names the big operand, the first small operand and the result like a
 * pair step; word 43 points at a descriptor in the table blob (geometry of the
 * tile decomposition, the second small operand, 14 offset tables: layout in
 * cotengra_amd/stem.py: serialise_stem, csrc/ctg_common.h: StemWord).  Like every
 * step it is validated by ctg_plan_create: tables inside the blob, every operand
 * address inside its buffer, a tile shape the kernel takes.
 *
 * ABI 7 -- LDS-resident subtrees (the small-tree execution model; the reference's step
 * loop contract.py:788-832 for a whole subtree at once).  Word 44 of a pair / single
 * step record: component id + 1 (0: none), word 45: word offset of the component's
 * descriptor in the table blob (cotengra_amd/ldsrun.py: serialise_run, csrc/ctg_common.h:
 * LdsHeadWord / LdsRecWord) -- a second lowering of the component's member steps on
 * tensors that live in one compute unit's LDS.  The member records stay complete and
 * come first in the step order; an executor runs all components of a plan as ONE launch
 * (one workgroup per component and slice of the batch) at the position of their first
 * member, or -- under strip_exponent, CTG_NO_LDS_RUNS=1, or when a component does not
 * fit the LDS of the device -- the member steps one by one.  ctg_plan_create validates
 * the descriptors like everything else (tables inside the blob, LDS addresses inside
 * the component's data area, global addresses inside their space).
 *
 * ABI 8 -- gradients (cotengra_amd/vjp.py: compile_vjp).  A VJP plan's inputs are the
 * leaves and the cotangent; it ends each slice with one accumulate step (kind 2) per
 * leaf whose result operand names THAT leaf (word 10 = i < n_inputs): the executor adds
 * leaf i's slice offset, and the coefficient that undoes the upload scaling of
 * single-precision inputs leaves input i's own power of two out (d O / d x_i carries
 * every other input's).  A forward plan's accumulate names the pseudo-leaf n_inputs and
 * keeps the whole coefficient.  A run of consecutive accumulate steps goes out as ONE
 * launch (accum_group_kernel, workgroups dealt in proportion to the steps' rows; the
 * same bits as one launch per step); ctg_plan_create rejects a plan whose consecutive
 * accumulate steps write overlapping result ranges.  A plan with one accumulate step
 * launches accum_kernel as before.
 *
 * Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION (a new kernel code, no new symbol; plans without it are
 * unchanged): kernel code 2 in word 1 of a pair record (kind 1) -- the sparse root step of a pick plan
 * (cotengra_amd/plan.py: compile_tree(pick=...), csrc/ctg_pick.hip).  Such a record has
 * N = 1, Bt = 1 and row_lo = 1: its R rows are requested members of the tree's output, the `hi` level of the
 * three row tables holding, per request, its offset in A, in B and its position in the result of the step,
 *   C[rowC(m)] = alpha * sum_k A[rowA(m) + kA(k)] * B[rowB(m) + kB(k)],
 * and the plan's result is the vector of the requests (result_elems = R).  ctg_plan_create rejects code 2 on any
 * other kind of record, with other extents, or with a row, k or n table absent (offset -1) (CTG_E_INVALID), and checks the per-request tables like every table
 * (sum of the table maxima per operand inside its space).  The step launches alone, carries the slices of a
 * batch like every thread-per-output step, and takes strip_exponent / check_zero like every pair step.
 *
 * Likewise added to ABI 10 without a bump: kernel code 3 in word 1 of a pair record -- the step of a row-sparse node
 * below the root of a chained pick plan (compile_tree(pick=..., pick_chain=...), csrc/ctg_pick_rows.hip, DESIGN.md
 * section 14).  Such a record has Bt = 1 and the tables of a thread-per-output pair step; its R = rows * row_lo rows
 * are the rows of the node (the `hi` level of the three row tables: per row the offset of its sub-tensor in A, in B
 * and in the result) times the row_lo dense positions A carries (the `lo` level), the n tables running over the N
 * positions only B carries,
 *   C[rowC.hi[m] + rowC.lo[i] + nC[n]] = alpha * sum_k A[rowA.hi[m] + rowA.lo[i] + kA(k)]
 *                                                      * B[rowB.hi[m] + rowB.lo[i] + kB(k) + nB[n]].
 * ctg_plan_create rejects code 3 on any other kind of record, with Bt != 1, or with a row, k or n table absent
 * (CTG_E_INVALID), and checks the per-row tables like every table.  The step launches alone and carries the slices
 * of a batch in gridDim.y.
 *
 * Words of a step record -- what ctg_plan_create holds each of them to (the layout is in cotengra_amd/plan.py:
 * Plan.serialise; tests/plan_words.py states the same word by word, for the stem and LDS descriptors as well, and
 * tests/test_plan_validation.py attacks every word with the hostile values of its class).  A descriptor is not trusted:
 * a word that is accepted can be turned into a host or device address without another look.
 *   enums          word 0 kind 0..3, word 1 kernel 0..3 (1 on pair steps only, 2 and 3 as above), word 42 sharing 0..2,
 *                  word 44 LDS component id + 1 (0 .. number of steps, a component with a valid descriptor).
 *   operands       A (words 2-4, 30), B (5-7, 31), C (8-10, 32): space (0 inputs, 1 arena, 2 result; C never 0), element
 *                  offset, leaf (-1; an input i whose slice offset moves the operand; n_inputs: the result's chunk offset)
 *                  and size.  [offset, offset + size) lies inside the space, size >= 1, and every address the tables
 *                  form -- the leaf's largest slice offset plus the largest entry of every table of the operand -- lies
 *                  inside [0, size): for a leaf, size is that of the whole tensor its slices lie in.  An operand the step
 *                  does not have (B of kinds 0 and 2) is written as space -1, offset 0, leaf -1, size 0, nothing else.
 *   extents        R, Bt, K, N (11-14) and the splits row_lo, row_hi_len (15, 16), k_lo, k_hi_len (36, 39): all >= 1,
 *                  row_lo * row_hi_len = R, k_lo * k_hi_len = K; Bt <= 65535, and Bt = 1 off the matrix-core kernels;
 *                  N = 1 on kinds 0 and 2, K = 1 on kind 2.  A kind-3 record restates its descriptor: R the rows of the
 *                  result over all tiles, K and N those of the last step, Bt and the four splits 1.
 *   tables         word offsets into the blob, lengths in brackets: rowA/B/C_hi (17, 19, 21) [row_hi_len], rowA/B/C_lo
 *                  (18, 20, 22) [row_lo], kA/kB_hi (37, 38) [k_hi_len], kA/kB_lo (23, 24) [k_lo], nB, nC (25, 26) [N],
 *                  bA, bB, bC (27-29) [Bt].  Who reads which: every ordinary step the A and C row tables; kinds 0 and 1
 *                  the kA tables; kind 1 the kB and n tables; kind 1 off the matrix cores (kernels 0, 2, 3) the B row
 *                  tables; kernel 1 the b tables; a kind-3 record none.  A table that is read lies inside the blob with
 *                  its whole length, its entries in [0, 2^56], and is present (>= 0) -- except that on the thread-per-
 *                  output route (kernel 0, on a step of any kind: single-term, pair or accumulate) a table of length 1
 *                  may be absent (negative): the executor reads one zero word instead.  Kernels 1, 2 and 3 have host
 *                  code that indexes their tables: nothing they read may be absent.  A table that is not read is absent
 *                  or points into the blob.
 *   step indices   a.producer, b.producer (40, 41): a pair or stem step, or anything outside [0, n_steps) -- "no
 *                  producer", scale factor 1; tolerated by design.
 *   descriptors    word 43 (kind 3): STEM_WORDS words inside the blob; word 45 (word 44 > 0): the component's header
 *                  and records inside the blob.  Free on every other record.
 *   free           macs, elems_rw, node (33-35), reserved (46, 47): read by nothing.
 * Sums of the caller's numbers are never formed unchecked: every term of an address is held to [0, 2^56] first, slice
 * offsets (stride x (extent - 1)) are multiplied with an overflow check, and the slices of every leaf lie inside it.
 * The stem descriptor's tables are never absent, its second small operand (a single step: space 0, offset 0, leaf -1,
 * size 0) and its middle stage (none: zeros) follow the operand rule; an LDS record's tables are never absent where the
 * packer reads them (all of a pair record; the A, C and kA tables of a load), its operands lie inside the component's
 * data area or, on the global side, inside the member step's space, R * ceil(N / 4) and R * K * N fit 32 bits, and
 * no record reads or writes the LDS range another record of the same phase writes.
 *
 * Changed in ABI 10 WITHOUT a bump of CTG_ABI_VERSION (no symbol, no layout and no plan of cotengra_amd/plan.py changes):
 * ctg_plan_create REFUSES descriptors it used to accept.  Besides the holes that were never meant to pass (a negative
 * word for a table that is read, size words, the b tables and the B row tables nobody checked, LDS record tables, sums
 * that wrapped), a caller that writes its own descriptors must know that these are now pinned, so that every word has
 * exactly one verdict:
 *   - Bt = 1 on every step that does not run on the matrix cores; N = 1 on single-term and accumulate steps, K = 1 (and
 *     both k splits 1) on accumulate steps;
 *   - an operand a record does not have is space -1, offset 0, leaf -1, size 0 (0 / 0 / -1 / 0 for the second small
 *     operand of a single stem step and for B of an LDS load record, whose LDS flag is 0);
 *   - the extent words of a kind-3 record restate its descriptor (R, K, N as above; Bt and the four splits 1);
 *   - the middle-stage words of a stem descriptor without a middle stage (34-38, 40-47) are zeros;
 *   - size words are >= 1 and [offset, offset + size) lies inside the space; table entries are never negative;
 *   - slice_fixed is -1 or a projected value >= 0; the largest slice offset of every leaf lies inside the leaf. */
typedef struct ctg_plan_desc {
    int32_t dtype;                /* CTG_F32 .. CTG_C128 */
    int64_t n_inputs;
    const int64_t* input_sizes;   /* [n_inputs] elements of each unsliced input */
    const int64_t* input_offsets; /* [n_inputs] element offset inside the inputs space */
    int64_t inputs_elems;         /* size of the inputs space */
    int64_t arena_elems;          /* size of the intermediates arena */
    int64_t result_elems;         /* size of the full output tensor */
    int64_t n_steps;
    const int64_t* steps;         /* [n_steps * CTG_STEP_WORDS], layout in plan.py */
    int64_t n_table_words;
    const int64_t* tables;        /* offset-table blob addressed by the step records */
    int64_t n_sliced;
    const int64_t* slice_sizes;   /* [n_sliced] extent (1 when projected) */
    const int64_t* slice_fixed;   /* [n_sliced] projected value or -1 */
    const int64_t* slice_strides; /* [(n_inputs+1) * n_sliced] element strides; row
                                     n_inputs is the output tensor (outer slices) */
    /* ABI 5 (may be NULL = none).  [n_sliced] 1: a GROUP index.  Slices that differ only in the group
     * indices form a group; a step whose record says so (word 42 = 2) depends on none of them and is
     * computed for the first slice of a group only, what later steps read of it living in arena ranges
     * no per-slice step writes (the planner's job, cotengra_amd/plan.py: choose_slice_group).
     * ctg_exec_run_slices visits the slices it is given group by group.  The reference recomputes every
     * slice from the leaves (core.py:3802-3834). */
    const int64_t* slice_group;
} ctg_plan_desc;

typedef struct ctg_plan ctg_plan;
typedef struct ctg_exec ctg_exec;
typedef struct ctg_comm ctg_comm;

/* Library / error --------------------------------------------------------- */
int ctg_abi_version(void);
const char* ctg_last_error(void);

/* Plan: host-only, needs no GPU.  Replaces building a `Contractor` from
 * `extract_contractions(tree)` (contract.py:994-1000).  The descriptor is
 * validated (kinds, table ranges, that every address stays inside its
 * buffer) and deep-copied. */
int ctg_plan_create(const ctg_plan_desc* desc, ctg_plan** out);
int ctg_plan_destroy(ctg_plan* plan);
/* number of independent slices = prod(slice_sizes) (core.py:403-408) */
int ctg_plan_nslices(const ctg_plan* plan, int64_t* nslices);
/* device bytes an exec will allocate: [0] inputs [1] arena [2] result
 * [3] tables+misc */
int ctg_plan_workspace_bytes(const ctg_plan* plan, int64_t bytes[4]);

/* Exec: one per GPU.  Owns inputs space, arena, tables; the result buffer is
 * either owned or caller-provided device memory (`ext_result`, e.g. memory a
 * collective library will reduce in place).  Replaces the lazy `setup(*arrays)`
 * of the whole-tree backend (contract.py:883-899).
 * A single-slice arena of 32 GiB or more is allocated twice where the free device memory allows
 * (peak: twice its size for a moment), the plan's largest tensors' ranges are read in both copies and
 * the faster copy is kept -- physical placement in HBM is worth 2-3 % of a slice on MI355X
 * (profiles/r6_process_alternation.txt); results do not depend on it.  CTG_ARENA_PLACE=0: off. */
int ctg_exec_create(const ctg_plan* plan, int device, void* stream,
                    void* ext_result, ctg_exec** out);
int ctg_exec_destroy(ctg_exec* exec);
/* Move the executor to another stream of its device (a caller that works under
 * changing stream contexts, e.g. `torch.cuda.stream(...)`): waits for the work
 * already enqueued on the old stream, then every later call enqueues on
 * `stream`. */
int ctg_exec_set_stream(ctg_exec* exec, void* stream);

/* Make the (unsliced) input tensors resident: `ptrs[i]` points to
 * input_sizes[i] contiguous row-major elements.  Replaces passing `*arrays`
 * to the contractor (contract.py:718, 779-780) / `reset_operands`
 * (contract.py:916).  `_host` synchronises the stream before returning;
 * `_device` enqueues device-to-device copies.
 * An executor may be uploaded and run any number of times: what it returns for
 * (inputs uploaded, arithmetic and options set, slices asked for) is the same
 * bits as a new executor of the same plan would return for them, whatever was
 * uploaded, run or set on it before. */
int ctg_exec_upload_inputs_host(ctg_exec* exec, const void* const* ptrs);
int ctg_exec_upload_inputs_device(ctg_exec* exec, const void* const* ptrs);

/* result <- 0 (start of a `gather_slices` reduction, core.py:3842-3844) */
int ctg_exec_zero_result(ctg_exec* exec);

/* strip_exponent / check_zero of the reference's Contractor (contract.py:
 * 674-683, 816-829): after every pairwise step the intermediate is normalised
 * by factor = max|p| and log10(factor) accumulated.  On the device the
 * normalisation is lazy (the consumer's epilogue multiplies by 1/(fac_l fac_r))
 * and slices are combined with the exponent-aware adder of core.py:125-172.
 * With strip on, the result tensor holds the mantissa and ctg_exec_get_exponent
 * returns the base-10 exponent E (result = mantissa * 10^E; E = -inf and
 * *zero = 1 when check_zero met a zero intermediate in every slice).  A plan
 * without a pairwise step (a one-input tree) has nothing to normalise: its
 * exponent is what the upload took out of the input, and check_zero tests the
 * slice output itself, so an all-zero result is (0, -inf) there too. */
int ctg_exec_set_strip_exponent(ctg_exec* exec, int strip_exponent, int check_zero);

/* Arithmetic of the fused stem pairs (step kind 3) of this executor.  1 (the default since ABI 4):
 * every fp32 operand of a pair is split EXACTLY into three bfloat16 values and the six significant
 * cross terms are accumulated in fp32 on the bf16 matrix cores (error bound,
 * domain -- operands above 2^-110, small operands rescaled by a power of two inside the kernel --
 * and the adversarial tests that hold it to the fp32 kernel's own error); the same accuracy against
 * a double-precision reference as 0, not the same bits, 11-13 % less time per slice.  0: complex64 on
 * the fp32 matrix cores, an exact-fp32 multiply-add chain like every other step.  The environment
 * variable CTG_STEM_BF16X3, when set, overrides the option ("0" = fp32).  No reference counterpart
 * (the reference computes in whatever its array library does).  Takes effect from the next run.
 * 2 (ABI 7, the default of a new executor unless CTG_STEM_ARITH = fp32 | bf16x3 | fp16x2 says otherwise):
 * two ROUNDED fp16 limbs per operand (22 bits) under per-tensor power-of-two scales and THREE products --
 * half the matrix work of 1, the stem pairs at 0.7 instead of 0.45 of the HBM roofline.  The scales: the
 * small operands' largest elements (found in-kernel), the big operand's as its producer recorded it (every
 * such kernel tracks the largest element it stores; a big operand of other origin gets a max-abs pass), the
 * intermediate tile's own; an element more than 2^-14 below its tensor's largest loses low bits gradually
 * (absolute error <= 2^-24 of the largest: norm-wise accuracy).  strip_exponent runs
 * and CTG_STEM_H2=0 fall back to 1.  The LONG TILED steps (K >= 64 on full 64-column tiles: the GEMM-like steps of
 * a tree) follow the same mode: 1 = six bf16 products, 2 = two fp16 limbs per value under ONE power of two per
 * operand tensor and slice, three products -- for a launch without k-splits (its operands' largest elements as
 * their producers recorded them per slice of the batch, else a max-abs pass); k-split launches and CTG_PAIR_H2=0
 * keep 1. */
int ctg_exec_set_stem_arithmetic(ctg_exec* exec, int mode);
int ctg_exec_get_exponent(ctg_exec* exec, double* exponent, int* zero);

/* Contract slices first, first+stride, ... (count of them) and ACCUMULATE each
 * into the result tensor at its chunk position: the slice loop of
 * `ContractionTree.contract` (core.py:4015-4030) fused with `gather_slices`
 * (core.py:3825-3882), or with count=1 `contract_slice` (core.py:3821-3823);
 * `stride = world_size` gives the round-robin of `contract_mpi`
 * (core.py:4068-4076).  Slice-to-leaf indexing (`slice_arrays`,
 * core.py:3802-3819) happens on the device. */
int ctg_exec_run_slices(ctg_exec* exec, int64_t first, int64_t count, int64_t stride);

/* How many slices of a run_slices call share one launch sequence.  A slice of a
 * narrow tree is launch-bound (Sycamore m10: 170 launches of a few microseconds),
 * so the executor carries up to `batch` consecutive slices of a run through every
 * launch (gridDim.y), each in its own replica of the arena; the reference's slice
 * loop (core.py:4015-4028) has no counterpart -- it is one Python iteration per
 * slice.  Chosen when the executor is built: min(64, nslices), bounded by 8 GiB
 * (and a quarter of the free device memory) of arena replicas (environment:
 * CTG_SLICE_BATCH, CTG_SLICE_BATCH_MIB); wide trees get 1.  The result does not
 * depend on it bit for bit: the k-split of every step is a function of the plan
 * (the step's shape and the plan's nominal batch min(64, nslices, 8 GiB / arena)
 * -- not of the environment, the free memory or the launch at hand), the kernels
 * and the order in which slices are added are those of one launch sequence per
 * slice. */
int ctg_exec_slice_batch(ctg_exec* exec, int64_t* batch);
/* ABI 5.  The same for an arbitrary list of slice ids (each in [0, nslices); repetitions allowed: a slice
 * given twice is added twice).  With slice groups in the plan (ctg_plan_desc.slice_group) the slices are
 * visited group by group and the steps a group shares are computed once per group among the ids given --
 * pass whole groups to get the saving; the sum does not depend on the grouping beyond the order of
 * its floating-point additions. */
int ctg_exec_run_slice_list(ctg_exec* exec, const int64_t* ids, int64_t n);
/* ABI 6.  A rank's SHARE of the slices, as the library deals them: the units rank, rank + world, ... where a
 * unit is a whole slice group (ctg_plan_desc.slice_group; what a group shares is then computed once per
 * group on exactly one rank) and, for a plan without group indices, a single slice -- which is the
 * round-robin `range(rank, nslices, size)` of contract_mpi (core.py:4068-4076).  The shares of the ranks
 * are disjoint, cover every slice and differ by at most one unit.
 *   ctg_plan_share_units      -> how many units rank holds and the slices in a unit (host only);
 *   ctg_plan_share_slice_ids  -> the slice ids of units [unit_first, unit_first + unit_count) of the
 *                                share, unit after unit, ascending inside a unit (unit_count < 0: to the
 *                                end; `ids` holds unit_count * slices_per_unit words) (host only);
 *   ctg_exec_run_share        -> contract those units and accumulate them like ctg_exec_run_slices; host
 *                                memory stays bounded by a chunk of groups whatever nslices is.
 * A checkpointing caller counts finished UNITS of its share and resumes with unit_first = that count. */
int ctg_plan_share_units(const ctg_plan* plan, int64_t rank, int64_t world, int64_t* units, int64_t* slices_per_unit);
int ctg_plan_share_slice_ids(const ctg_plan* plan, int64_t rank, int64_t world, int64_t unit_first,
                             int64_t unit_count, int64_t* ids);
int ctg_exec_run_share(ctg_exec* exec, int64_t rank, int64_t world, int64_t unit_first, int64_t unit_count);
/* ABI 4.  Device memory this executor holds right now: inputs space, arena x slice batch,
 * tables, the result if it owns it, the scratch buffer if the plan has a step that needs one
 * (allocated by ctg_exec_create), the scratch of ctg_exec_result_stats / ctg_exec_sample_result once they
 * have run (ABI 9), of ctg_exec_range_audit and of ctg_exec_result_topk / ctg_exec_result_marginal / ctg_exec_result_rdm /
 * ctg_exec_result_pauli likewise (ABI 10).  What a cache of contractors -- the reference keeps them
 * on the tree, core.py:3708-3722 -- has to count against its budget. */
int ctg_exec_device_bytes(ctg_exec* exec, int64_t* bytes);
/* ABI 5.  Is there a kernel instantiation for a three-step tile of this shape (stem steps fused
 * three at a time, cotengra_amd/stem.py: build_stem_triple; opt-in, CTG_STEM_TRIPLES)?  A pure
 * function of the shape -- 16 output columns in the first / middle / last step (0 / 1), units of
 * step 1 per wave, its column groups, 16-deep chunks of its contraction, work items per wave of the
 * middle and of the last step, 16-byte gathers (0 / 1) -- that needs no device: the planner asks
 * before it emits such a record (there is no run-time-count variant; ctg_plan_create rejects a
 * record without one).  Returns 1 or 0.  (The reference has no counterpart: it contracts step by
 * step, contract.py:788-832.) */
int ctg_stem_triple_instantiated(int p1, int pm, int p2, int rt1, int cs1, int nch, int itm, int it2, int vec);

/* Steps of one slice and the kernel launches they take.  Independent small steps
 * (the leaves-upward wave fronts of a tree; the reference contracts them one
 * einsum call after the other, contract.py:788-829) share launches: `steps` pair /
 * single / accumulate steps per slice go out as `launches` launches.  Grouping
 * never changes a result bit (every output element is computed by the same
 * thread in the same order); it is off under strip_exponent and with the
 * environment variable CTG_NO_GROUPS. */
int ctg_exec_launch_count(ctg_exec* exec, int64_t* steps, int64_t* launches);

/* Same as run_slices(slice_id, 1, 1) but brackets every step with events and
 * returns its duration in milliseconds (`ms[n_steps]`); synchronous.  Serves
 * the role of `tree.print_contractions` + `tree.benchmark`
 * (core.py:3508, 4092-4164) for per-step rooflines. */
int ctg_exec_profile_slice(ctg_exec* exec, int64_t slice_id, float* ms);

/* Name of the kernel that executes plan step `step` on this executor (e.g.
 * "pair_mfma_fast_kernel<128,128,16>"), NUL-terminated into `buf`; lets a
 * profile attribute per-step timings to rocprof kernel names.  The name is the
 * profiler's, shortened: no namespace, no argument list, template arguments as the
 * launcher chose them for a launch of one slice.  Pair steps in float32, float64
 * and complex128 spell out tile and gather width:
 *   "pair_mfma_c128_kernel<TM,TN>"                           e.g. <4,2>
 *   "pair_mfma_real_kernel<float|double,TM,TN,true|false>"   (last: 16-byte gathers)
 * complex64 pair steps on the matrix-core route are one of
 *   "pair_mfma_stream_kernel<FN,VEC,ADD,SHORTK,NV>"          e.g. <1,true,true,false,8>
 *   "pair_rowwise_kernel<NN,TS>"                             e.g. <8,true>
 *   "pair_skinny_kernel<K,N>"
 *   "pair_mfma_kstream_kernel<FN,VEC> + splitk_reduce_kernel[S]"
 *   "pair_mfma_{c64|fast|bf3|h2}_kernel<128,BN,16>,VEC"      tiled, one pass over k
 *   "pair_mfma_{c64|fast|bf3}_kernel<128,BN,16>,VEC + splitk_reduce_kernel[S]"
 * (S > 1 slabs of partial sums per output and the pass that adds them);
 * and the steps of every type that do not run on the matrix cores are
 *   "pair_valu_kernel"                                       a thread per output
 *   "pair_kred_kernel + pair_kred_finish_kernel<true|false>" lanes along a long k
 *   "pair_kred_multi_kernel<2|3|4> + pair_kred_finish_kernel<true|false>"
 * (two launches: the partial sums and the pass that adds them, a wavefront per
 * output when <true>).  The sparse root step of a pick plan (kernel code 2) is
 *   "pair_pick_kernel<float|double|c64|c128,VEC,SEG>"        VEC 1 | 2 adjacent k per load, SEG lanes per request
 * or, few requests under a very long contraction, one of the two k-reduction names above.  A row-sparse step
 * below the root (kernel code 3) is
 *   "pair_pick_rows_kernel<float|double|c64|c128,VEC>"       vector form, VEC 1 | 2 adjacent k per load
 *   "pair_pick_rows_mfma_kernel<c64>"                        matrix-core form (row_lo >= 32, N >= 8, K >= 8)
 * A single-term step (diagonal, trace, sum, transpose, the preprocessing of a leaf) is
 *   "single_wave_kernel"                                     a wave per output, lanes along the sum (K >= 256, R <= 2^14)
 *   "single_kernel"                                          a thread per output (everything else)
 * and the slice sum "accum_kernel" ("accum_group_kernel": gradients sharing a launch).
 * Match by prefix. */
int ctg_exec_step_kernel(ctg_exec* exec, int64_t step, char* buf, int64_t buflen);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION: one new symbol, nothing else changes.
 * The members of an LDS-resident subtree are all "lds_run_kernel[c]" above; inside that launch every shadow record of
 * packed component c takes one of several forms, decided by the packer.  Record `rec` (in the order the workgroup
 * walks them) of component `comp` is
 *   "load<gather|sum> DEAL DIV"          global -> LDS: a plain gather (K = 1), or a gather that sums (leaf trace /
 *                                        diagonal / sum)
 *   "pair<1|2|4> DEAL DIV"               a pair step on the vector units, 1, 2 or 4 columns per lane
 *   "pair_mfma<cols|rows> DEAL DIV"      a complex64 pair step on the matrix cores, columns or rows on the lanes
 * DEAL is "wave=W", the one wave the record is dealt to, or "all", shared by the workgroup's sixteen waves -- a
 * matrix-core record then "all rot=R", the wave its first tile goes to; DIV is "shift" or "magic", how a row number
 * is divided by the length of the low row table (a shift; or the high half of a product with
 * floor(2^32 / row_lo) + 1).  *main_step is the plan step the record belongs to.  A record past the component's last,
 * and a component past the last packed one -- which includes every component the packer left off (CTG_NO_LDS_RUNS,
 * strip_exponent, a blob that does not fit) --, gives an empty name and *main_step = -1. */
int ctg_exec_lds_form(ctg_exec* exec, int64_t comp, int64_t rec, int64_t* main_step, char* buf, int64_t buflen);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION: THREE new symbols, nothing else changes -- a plan, an executor and
 * every existing call behave as before, which is the rule by which ABI 10 has grown (kernel codes 2 and 3, top-k,
 * marginals, reduced density matrices); the binding binds them like every other symbol.
 * A stem pair whose consumers hold both 32-column groups of a row tile stores two adjacent columns of a row as one
 * 16-byte store where the step's own tables allow it: the paired columns exactly one element apart, every row, tile and
 * slice offset and the result's place in its space even.  The kernel is then the symbol "stem2h_kernel_p16<...>" in a
 * trace, with the template arguments of the "stem2h_kernel<...>" that ctg_exec_step_kernel goes on naming; results are
 * bit for bit those of the 8-byte form.  *paired = 1 if the step's LAST launch took that form -- recorded by the
 * launcher itself --, else 0 (a step that has not run, and any other kind of step, included).  CTG_STEM_NO_PAIR16=1 in
 * the environment (a diagnostic switch, read per launch) keeps every step on 8-byte stores. */
int ctg_exec_step_paired_stores(ctg_exec* exec, int64_t step, int* paired);
/* The largest |real or imaginary part| that the last launch of stem step `step` recorded of what it stored, for slice `z`
 * of the batch (0 for a step that slices share): what a consumer in the fp16 x 2 arithmetic scales its split with.
 * Synchronises the stream.  CTG_E_INVALID for a step that is no stem step or whose last launch recorded nothing (fp32
 * products, strip_exponent). */
int ctg_exec_step_stem_max(ctg_exec* exec, int64_t step, int64_t z, float* mx);
/* The verdict on the tables alone, of a plan in host memory: *ok = 1 if step `step` is
 * a stem pair whose result's tables meet the condition above, else 0.  Which kernels then use it is the launch's
 * business (shape, arithmetic and form of the step: ctg_exec_step_paired_stores). */
int ctg_plan_stem_pair16(ctg_plan* plan, int64_t step, int* ok);

int ctg_exec_sync(ctg_exec* exec);
/* device address of the result tensor (result_elems elements, row-major in
 * the tree's output index order) */
int ctg_exec_result_ptr(ctg_exec* exec, void** dev_ptr);
/* synchronous copy of the result to host memory */
int ctg_exec_download_result(ctg_exec* exec, void* host_out);
/* ABI 9.  What a caller wants from an amplitude batch (a tree with open output qubits; quimb's
 * `Circuit.sample_chaotic` on top of the reference) without moving the batch to the host: statistics of, and draws
 * from, p_i = |x_i|^2 over the result tensor -- result_elems elements, row-major in the tree's output order, whoever
 * owns the memory -- as it stands after the work already enqueued on the executor's stream.  p is formed and summed
 * in double for every element type (re*re + im*im; an fp32 square of a deep circuit's amplitude is zero), by three
 * kernels of fixed summation order (csrc/ctg_sample.hip): the same tensor and the same
 * uniforms give the same bits on every run and every executor.  Both calls synchronise the stream.  For a
 * single-precision sliced tree they read the result tensor (the double-precision sum of the slices rounded once),
 * not the wide sum.  There is no multi-rank entry: after ctg_exec_reduce the root's (every rank's, for an
 * all-reduce) result tensor holds the total and the same calls work there.  Not differentiable.
 * The scratch (40 bytes per 4096 elements, 40 per draw of a chunk of at most 2^18) is allocated by the first call,
 * grown on demand, counted by ctg_exec_device_bytes and freed by ctg_exec_destroy. */
/* sum|x|^2, sum|x|^4, max|x|^2 and its (lowest) flat index over the result tensor, in double (each may be NULL).
 * Under strip_exponent the values are the mantissa's; the true ones are x 10^(2E), 10^(4E), 10^(2E). */
int ctg_exec_result_stats(ctg_exec* exec, double* sum_p, double* sum_p2, double* max_p, int64_t* argmax);
/* n draws from p_i / sum p by inverse CDF: u[s] in [0,1) (host) -> idx[s] (host, flat row-major index): the
 * element at which the running sum of p first exceeds u[s] * sum p, up to the rounding of two summation orders
 * (|error| <= 2 * result_elems * 2^-53 * sum p on that target); never an element with p = 0.  Where non-NULL,
 * elems[s] (plan dtype) and p[s] (double) receive the element at idx[s] and its p.  CTG_E_INVALID for a null
 * exec / u / idx, n < 0, a uniform outside [0,1) or NaN -- checked on the host before anything is launched;
 * CTG_E_NORM when sum p is zero or not finite.  n = 0 succeeds and does nothing.  The uniforms are the caller's:
 * the call is a pure function of (result tensor, u), the generator is the host's choice. */
int ctg_exec_sample_result(ctg_exec* exec, const double* u, int64_t n, int64_t* idx, void* elems, double* p);
/* What the last ctg_exec_result_stats / ctg_exec_sample_result call on this executor found -- the four statistics
 * of the tensor AS IT WAS THEN (a caller that has just drawn needs no second pass over the tensor for its norm) --
 * and, where pass_ms is non-NULL, pass_ms[0..1]: the device time in milliseconds of that call's pass 1
 * (prob_block_kernel) and pass 2 (prob_scan_kernel), from events on the executor's stream.  Any pointer may be NULL.
 * CTG_E_INVALID when no such call has completed.  Host only: launches and copies nothing. */
int ctg_exec_sample_info(ctg_exec* exec, double* sum_p, double* sum_p2, double* max_p, int64_t* argmax, float* pass_ms);
/* ABI 10.  Range audit (csrc/ctg_range.hip): where the components of every tensor of one slice
 * lie below the tensor's largest one.  The fp16 x 2 arithmetic keeps one power of two per operand tensor, so its
 * error is a fraction of the tensor's LARGEST element; this call measures what that means for the data at hand.
 * float32 and complex64 plans only (CTG_E_INVALID otherwise: double-precision trees have no reduced arithmetic), not
 * under strip_exponent (CTG_E_INVALID: the stored values are not the logical ones there, and fp16 x 2 is off).
 *
 * The call runs slice `slice_id` as ctg_exec_profile_slice does -- every step launched on its own, LDS-resident
 * subtrees as their one launch, slice-invariant steps once per upload, the executor's current arithmetic -- and adds
 * the slice into the result tensor, as run_slices(slice_id, 1, 1) would.  After every step whose result lies in the
 * arena it reads that result (its W_C_SIZE contiguous elements, as n fp32 components: 2 per complex64 element).
 * rows[(n_inputs + n_steps) * CTG_RANGE_WORDS] and sumsq[n_inputs + n_steps] (host) receive, for the input tensors
 * (rows 0 .. n_inputs - 1: the whole leaf as stored in the inputs space, after the upload's power-of-two scaling,
 * which moves all bins of a tensor together) and the result of step s (row n_inputs + s):
 *   word 0        1: audited; 0: not materialised (a member of an LDS-resident subtree, an accumulate step, a
 *                 result outside the arena) -- the other words are 0 then
 *   word 1        number of components
 *   word 2        components equal to +-0
 *   word 3        reserved (0)
 *   word 4 + b    components whose biased exponent field (bits >> 23) & 0xff is b: b = 0 zeros and subnormals,
 *                 b = 255 inf and NaN
 *   sumsq         sum of x^2 over the finite components, each square formed in double, summed in a fixed order
 * The same bytes give the same numbers on every run and on every executor (integer counts; no float atomics).
 * Before every pass the host checks offset + size of the tensor against its space: CTG_E_BOUNDS, nothing is read.
 * CTG_E_INVALID for null pointers and a slice id outside [0, nslices).  Synchronous.  The pass only reads; a later
 * call returns what it would return on an executor that had run the slice with run_slices.  The scratch (a few MiB
 * at most) is allocated by the first call, grown on demand, counted by ctg_exec_device_bytes and freed by
 * ctg_exec_destroy. */
#define CTG_RANGE_WORDS 260
int ctg_exec_range_audit(ctg_exec* exec, int64_t slice_id, int64_t* rows, double* sumsq);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION (two new symbols, nothing else changes; a binding that needs them
 * looks them up): the k most probable members, and marginals, of the result tensor on the device
 * (csrc/ctg_reduce.hip).  Both read the result tensor as ctg_exec_sample_result does --
 * result_elems elements, row-major, whoever owns the memory, the mantissa under strip_exponent, after the work already
 * enqueued on the executor's stream -- with the same p_i = |x_i|^2 in double, and synchronise the stream.  Both return
 * CTG_E_NORM when sum p (from the statistics passes of ABI 9, which they run first) is not finite: a NaN or inf
 * member.  An all-zero tensor is NOT an error here.  No floating-point atomics; every grid and every association of a
 * sum is a function of (result_elems, k) / (extents, keep): the same bytes give the same bits on every run and every
 * executor.  The scratch is allocated by the first call, grown on demand, counted by ctg_exec_device_bytes and freed
 * by ctg_exec_destroy.  Not differentiable; no multi-rank entry (as for ABI 9). */
/* The first k members of the order (p descending, lower flat index first among equal p), in that order: idx[k], and
 * where non-NULL elems[k] (plan dtype) and p[k].  Exact: numpy's lexsort((index, -p))[:k] index for index, p bit for
 * bit.  A radix select on the bit pattern of p (12-bit digits; on a compact list of the surviving keys once at most
 * 2^16 survive), a collection in index order, and the ordering of the k records on the host inside the call.
 * CTG_E_INVALID for k < 1, k > result_elems, k > CTG_TOPK_MAX or a null exec / idx -- checked on the host before
 * anything is launched.  Scratch: 16 MiB of digit counts at most, 24 bytes per 4096 elements, 512 KiB, 32 bytes per
 * record. */
#define CTG_TOPK_MAX (1 << 20)
int ctg_exec_result_topk(ctg_exec* exec, int64_t k, int64_t* idx, void* elems, double* p);
/* out[j] = sum of p over the elements whose kept coordinates are j: extents[rank] is the shape of the result (its
 * product must equal result_elems), keep[a] in {0, 1} selects the axes kept, out holds prod(kept extents) doubles,
 * row-major over the kept axes in the tensor's own axis order.  rank = 0 or no kept axis: out[0] = sum p; all axes
 * kept: out = p.  Every extent a power of two (and at least 4096 elements): per block of 4096 elements a tree over the
 * dropped bits, then the blocks of an output in ascending order in chunks of 64, the tensor in slabs of at most
 * CTG_MARGINAL_PARTIALS partial sums; any other shape: a serial walk per (output, chunk of 1024 complement positions).
 * |out[j] - exact| <= (t - 1) 2^-53 out[j] for the t elements of an output.  CTG_E_INVALID for a negative rank, a
 * non-positive extent, a wrong product, a keep value outside {0, 1} or null pointers.  Scratch: 8 bytes per output
 * and at most 2 * 8 * CTG_MARGINAL_PARTIALS bytes (general route: 8 bytes per 512 elements instead). */
#define CTG_MARGINAL_PARTIALS (1 << 22)
int ctg_exec_result_marginal(ctg_exec* exec, int64_t rank, const int64_t* extents, const int32_t* keep, double* out);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION likewise (one new symbol; a binding that needs it looks it up): the
 * reduced density matrix of the kept axes of the result tensor on the device (csrc/ctg_rdm.hip),
 *   rho[a, b] = sum over r of x[a, r] * conj(x[b, r]),
 * a, b over the kept axes, r over all the others.  extents[rank] and keep[a] in {0, 1} are those of
 * ctg_exec_result_marginal, which returns the diagonal of this matrix.  D = the product of the kept extents,
 * t = result_elems / D: out holds D * D elements, row-major -- double2 {re, im} for complex plans, double for real
 * plans (rho is real symmetric there) -- rows and columns row-major over the kept axes in the tensor's own order.
 * No kept axis: D = 1, out = sum p; all axes kept: t = 1, out = x x^dagger.  The tensor is read as the two calls
 * above read it (whoever owns the memory, the mantissa under strip_exponent, after the stream's earlier work, after
 * the statistics passes, which run first); the stream is synchronised.  CTG_E_NORM when sum p is not finite; an
 * all-zero tensor gives a zero matrix.  CTG_E_INVALID for everything ctg_exec_result_marginal refuses, a null out, and
 * D > CTG_RDM_MAX_DIM -- checked on the host before anything is launched.
 *   - The result is exactly Hermitian: only b <= a is computed, the other half is written as its conjugate, and
 *     Im rho[a, a] is exactly 0.0.
 *   - No floating-point atomics.  Every grid and every association of a sum is a function of (extents, keep) alone:
 *     the same bytes give the same bits on every run and every executor.
 *   - Every product is formed in fp64 -- exact for float / complex64 plans, rounded once for double plans -- and every
 *     sum is in fp64: per real component |rho[a,b] - exact| <= (m + 1) 2^-53 sqrt(rho[a,a] rho[b,b]) with m = 2t
 *     (complex) or t (real) products.
 * Every extent a power of two and at least 4096 elements: chunks of 4096 elements (all rows -- 16 at least: for D < 16
 * low bits of r are folded into the row and summed out at the end -- by 4096 / rows consecutive values of r), widened
 * to fp64 in LDS and multiplied by v_mfma_f64_16x16x4_f64 on the 16 x 16 tiles of the lower triangle; a workgroup takes
 * the chunks wg, wg + grid, ... in ascending order, grid = min(512, ceil(chunks / 3)); the workgroups' partial sums are
 * added in ascending order in groups of 32, then the groups.  The kernel is "rdm_chunk_kernel<T,NT>", T in
 * float | double | c64 | c128, NT = max(D, 16) / 16 in 1 | 2 | 4.  Any other shape: "rdm_general_kernel<T>", a serial
 * walk per (a, b <= a, chunk of max(1024, ceil(t / 1024)) values of r), the chunks added in ascending order; not
 * tuned.  Scratch: the buffer of the two calls above (counted by ctg_exec_device_bytes, freed by ctg_exec_destroy):
 * 16 D^2 bytes for the output, and at most 512 * 40 KiB of partial sums + 16 * 40 KiB of group sums (21 MiB;
 * general route: at most 1024 * 16 D^2 bytes, 64 MiB).  Not differentiable.  No multi-rank entry: after
 * ctg_exec_reduce the root's result tensor holds the total and the call works there (untested). */
#define CTG_RDM_MAX_DIM 64
int ctg_exec_result_rdm(ctg_exec* exec, int64_t rank, const int64_t* extents, const int32_t* keep, void* out);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION likewise (one new symbol; a binding that needs it looks it up):
 * expectation values of Pauli strings over the axes of the result tensor on the device (csrc/ctg_pauli.hip, DESIGN.md
 * section 16).  extents[rank] is the shape of the result (its product must equal result_elems); ops[m * rank],
 * row-major, gives every axis of every string one of I, X, Y, Z as 0, 1, 2, 3 (Y = [[0, -i], [i, 0]]); an axis that
 * is not I must have extent 2.  out[s], one double per string for every dtype, receives
 *   value(P) = sum over j of conj(x[j]) (P x)[j],
 * NOT normalised (the all-identity string gives sum p).  With xm the flat-index bits of the X and Y axes, zm those of
 * the Z and Y axes, ny the number of Y and S = sum over j of (-1)^popcount(j & zm) conj(x[j ^ xm]) x[j]:
 * value = (-1)^(ny/2) Re S for even ny, (-1)^((ny+1)/2) Im S for odd ny.  For real plans a string with odd ny is
 * exactly 0.0 and is written without a launch.  The tensor is read as the calls above read it (whoever owns the
 * memory, the mantissa under strip_exponent, after the stream's earlier work, after the statistics passes, which run
 * first); the stream is synchronised.  CTG_E_NORM when sum p is not finite; an all-zero tensor gives zeros.
 * CTG_E_INVALID -- checked on the host before anything is launched, the tensor untouched -- for a null exec, extents,
 * ops or out, rank < 0, an extents product other than result_elems, m < 0 or m > CTG_PAULI_MAX_STRINGS, a code above 3
 * and a non-identity code on an axis whose extent is not 2.  m = 0 succeeds and does nothing.
 *   - Every product is formed in fp64 -- exact for float / complex64 plans, rounded once for double plans -- and every
 *     sum is in fp64; no floating-point atomics.  |out[s] - exact| <= (t + 1) 2^-53 sum p with t = 2 result_elems
 *     (complex) or result_elems (real) products.
 *   - The bits of out[s] are a function of (dtype, extents, row s of ops, the tensor's bytes) alone: not of the other
 *     strings of the call, their order, earlier calls in the same scratch, or the executor.  One accumulator per
 *     string; grids and the dealing of chunks do not depend on how many strings share a pass.
 * The strings of a call are grouped by xm (groups in order of first appearance, the caller's order inside) and a group
 * runs in passes of at most 32 strings, each pass one read of the tensor: of every unordered pair {j, j ^ xm} one
 * member is summed and the sum doubled, exactly, at the end (xm = 0: the term is |x[j]|^2, every j is summed).  Every
 * extent a power of two and at least 4096 elements: "pauli_chunk_kernel<T>", T in float | double | c64 | c128 -- chunks
 * of 4096 elements (chunk pairs (c, c ^ (xm >> 12)) where xm reaches past a chunk), the partner from an LDS copy, the
 * signs from one 32-bit word per element and one per chunk, 32 fp64 accumulators per thread; a workgroup takes the
 * units wg, wg + grid, ... in ascending order, grid = min(512, ceil(units / 3)); lanes and waves are added in a fixed
 * order, the workgroups' partials in ascending order in groups of 32, then the groups.  Any other shape:
 * "pauli_general_kernel<T>", a serial walk per (string, chunk of max(1024, ceil(result_elems / 1024)) flat indices),
 * the chunks added in ascending order; not tuned.  Scratch: the buffer of the calls above (counted by
 * ctg_exec_device_bytes, freed by ctg_exec_destroy): 8 m bytes of values and 648 bytes per pass, 128 KiB of partials,
 * 4 KiB of group sums (2.8 MiB at most; general route: 32 bytes per string, 12 per non-identity letter, 8 per (string,
 * chunk): 35 MiB at most).  Not differentiable.  No multi-rank entry: after ctg_exec_reduce the root's result tensor
 * holds the total and the call works there (untested). */
#define CTG_PAULI_MAX_STRINGS 4096
int ctg_exec_result_pauli(ctg_exec* exec, int64_t rank, const int64_t* extents, int64_t m, const uint8_t* ops, double* out);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION likewise (one new symbol; a binding that needs it looks it up):
 * y = (sum over s of coeffs[s] P_s) x for Pauli strings P_s over the axes of the result tensor x, written on the device
 * (csrc/ctg_pauli_apply.hip).  H = sum c_s P_s is Hermitian and the contraction is holomorphic in
 * its leaves, so conj(2 y) is the cotangent of E = <x| H |x> for a VJP plan: energy and gradient stay on the device.
 * extents, ops[m * rank] and the codes 0 .. 3 are those of ctg_exec_result_pauli; coeffs[m] are real.  With xm the
 * flat-index bits of the X and Y axes of a string, zm those of its Z and Y axes and ny its number of Y,
 *   (P x)[j] = i^ny (-1)^popcount((j ^ xm) & zm) x[j ^ xm],     y[j] = sum over s of coeffs[s] (P_s x)[j],
 * result_elems elements of the plan's dtype, written to dev_out (device memory that does not overlap the result
 * tensor), to host_out (a synchronous copy) or to both; with host_out alone y is staged in the scratch of the calls
 * above (counted by ctg_exec_device_bytes, freed by ctg_exec_destroy).  The tensor is read as the calls above read it
 * (whoever owns the memory, the mantissa under strip_exponent, after the stream's earlier work, after the statistics
 * passes, which run first) and never written; the stream is synchronised.  CTG_E_NORM when sum p is not finite; an
 * all-zero tensor gives zeros.  CTG_E_INVALID -- checked on the host before anything is launched, the tensor and both
 * buffers untouched -- for everything ctg_exec_result_pauli refuses (out aside), null coeffs with m > 0, both outputs
 * null, a dev_out that overlaps the result tensor, a coefficient that is not finite and, on real plans, a string with
 * an odd number of Y (P x is not real).  m = 0 writes zeros.  m <= CTG_PAULI_MAX_STRINGS.
 *   - Arithmetic: the strings are grouped by their X / Y axis set (xm), groups in order of first appearance, the
 *     caller's order inside a group.  Per element j and group g a complex fp64 weight W starts at 0 and takes, string
 *     after string, +-coeffs[s]: into Re W for even ny, Im W for odd ny, negative when the parity of popcount(j & zm)
 *     and of (ny mod 4 in {1, 2}) differ.  Then, with p = x[j ^ xm_g] in fp64: acc_re += (Re W p_re - Im W p_im),
 *     acc_im += (Re W p_im + Im W p_re) -- four products, the difference / sum and the addition each rounded once,
 *     nothing fused; real plans: acc += W p.  After the last group acc is rounded once to the plan's dtype.
 *   - No atomics and no sum across threads: the bits of y are a function of (dtype, extents, ops in order, coeffs, the
 *     tensor's bytes) alone -- not of the executor, the grid, earlier calls in the scratch, or which output was asked.
 *   - Per real component |y[j] - exact| <= (m + 2) 2^-53 sum over s of |c_s| (|Re| + |Im|)(x[j ^ xm_s]) + u |y[j]|,
 *     u = 2^-24 for float / complex64 plans and 2^-53 for double / complex128 (first order).
 * Every extent a power of two and at least 4096 elements: "pauli_apply_kernel<T>", T in float | double | c64 | c128, one
 * launch: a workgroup takes the output chunks wg, wg + grid, ... of 4096 elements, grid = min(512, ceil(chunks / 3)); a
 * thread keeps 16 elements' acc and W in fp64 registers; a group's strings run in passes of 32, one sign word per
 * (element, pass); the partner chunk c ^ (xm >> 12) is read once per group, straight into registers or through an LDS
 * copy; y is written with one 16-byte store per lane and 16-byte group.  Any other shape:
 * "pauli_apply_general_kernel<T>", a thread per output element, same groups and order; not tuned.  Scratch: 1640 bytes
 * per pass (general route: 24 per group, 24 per string, 8 per non-identity letter) plus the staged y.  No multi-rank
 * entry: after ctg_exec_reduce the root's result tensor holds the total and the call works there (untested). */
int ctg_exec_result_pauli_apply(ctg_exec* exec, int64_t rank, const int64_t* extents, int64_t m, const uint8_t* ops,
                                const double* coeffs, void* dev_out, void* host_out);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION likewise (one new symbol; a binding that needs it looks it up):
 * y = (sum over t of O_t (x) 1) x for small dense matrices O_t on named axes of the result tensor x, of ANY extent,
 * written on the device (csrc/ctg_op_apply.hip): spin-1 sites, qutrits, boson modes, projectors,
 * hopping terms, arbitrary few-site observables.  With H = sum O_t Hermitian, conj(2 y) is the cotangent of E = <x| H
 * |x> for a VJP plan, as for ctg_exec_result_pauli_apply.  Term t acts on naxes[t] >= 1 distinct axes, given in
 * ascending axis position; axes[] is the concatenation over the terms; D_t is the product of the extents of term t's
 * axes.  mats holds, term after term, D_t x D_t complex entries as (re, im) pairs of doubles, rows and columns
 * row-major over the term's axes in that ascending order:
 *   y[a, r] = sum over t, b of O_t[a, b] x[b, r],     a, b over the term's axes, r over all others,
 * result_elems elements of the plan's dtype, written to dev_out, to host_out or to both with exactly the staging,
 * ownership, stream and scratch rules of ctg_exec_result_pauli_apply; the tensor is never written.  CTG_E_NORM when
 * sum p is not finite; an all-zero tensor gives zeros.  CTG_E_INVALID -- checked on the host before anything is
 * launched, the tensor and both buffers untouched -- for everything ctg_exec_result_pauli_apply refuses about exec,
 * rank, extents, the outputs and their overlap with the result tensor; m < 0 or m > CTG_OP_MAX_TERMS; null naxes, axes
 * or mats with m > 0; a term with no axis, an axis out of range, repeated or not ascending within a term; D_t >
 * CTG_OP_MAX_DIM (= CTG_RDM_MAX_DIM: every term's expectation value can come from one reduced density matrix); more
 * than CTG_OP_MAX_ENTRIES matrix entries (sum of D_t^2) in all; a matrix entry that is not finite and, on real plans, a
 * non-zero imaginary part.  m = 0 writes zeros.
 *   - Arithmetic: per element j a complex fp64 accumulator starts at +0; terms in the caller's order; inside a term b
 *     = 0 .. D_t - 1 ascending (ascending partner flat index, because the axes ascend).  With p = x[partner(j, b)] in
 *     fp64 and W = O_t[a(j), b]: acc_re += (W_re p_re - W_im p_im), acc_im += (W_re p_im + W_im p_re) -- four products,
 *     the difference / sum and the addition each rounded once, nothing fused; real plans: acc += W_re p.  After the last
 *     term acc is rounded once to the plan's dtype.  An entry that is zero in both parts may be skipped: it would add
 *     +-0 to an accumulator that is never -0, so for a finite tensor no bit changes.
 *   - No atomics and no sum across threads: the bits of y are a function of (dtype, extents, the terms in order, the
 *     tensor's bytes) alone -- not of the executor, the grid, earlier calls in the scratch, or which output was asked.
 *   - Per real component |y[j] - exact| <= (N + 2) 2^-53 sum over t, b of (|Re W| + |Im W|)(|Re p| + |Im p|) + u |y[j]|,
 *     N = sum of D_t, u = 2^-24 for float / complex64 plans and 2^-53 for double / complex128 (first order).
 * Every extent a power of two and at least 4096 elements: "op_apply_kernel<T>", T in float | double | c64 | c128, one
 * launch with the geometry of pauli_apply_kernel (256 threads, two workgroups per CU, chunks of 4096 elements, grid =
 * min(512, ceil(chunks / 3)), 16 elements' accumulators per thread).  A term's flat-index bits below 12 lie inside a
 * chunk, those above are uniform over it: per term the workgroup walks the partner chunks in ascending order, stages
 * each in LDS and reads its partners and the block of O_t (LDS when at most 8 KiB, else the scratch) from there; a
 * partner chunk whose whole block of O_t is zero is not read (a diagonal term reads the tensor once).  Any other shape:
 * "op_apply_general_kernel<T>", a thread per output element, same order; not tuned.  Scratch: 456 bytes per term
 * (general route: 88), 16 bytes per matrix entry (16 MiB at most), 8 bytes per block, plus the staged y.  No multi-rank
 * entry, as above. */
#define CTG_OP_MAX_DIM 64
#define CTG_OP_MAX_TERMS 4096
#define CTG_OP_MAX_ENTRIES (1 << 20)
int ctg_exec_result_op_apply(ctg_exec* exec, int64_t rank, const int64_t* extents, int64_t m, const int32_t* naxes,
                             const int32_t* axes, const double* mats, void* dev_out, void* host_out);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION likewise (two new symbols; a binding that needs them looks them up):
 * reduced density matrices of 65 .. CTG_RDM_WIDE_MAX_DIM rows of the result tensor on the device
 * (csrc/ctg_rdm_wide.hip): the cut of a 20 - 24 qubit state or a 12 - 14 site spin-1 chain.
 *   rho[a, b] = sum over r of x[a, r] * conj(x[b, r])
 * with extents, keep, D, t, the layout of out and the reading of the tensor exactly those of ctg_exec_result_rdm
 * (whoever owns the memory, the mantissa under strip_exponent, after the stream's earlier work, after the statistics
 * passes, which run first; the stream is synchronised; CTG_E_NORM when sum p is not finite; an all-zero tensor gives a
 * zero matrix and purity 0).  out (D * D double2, or double for real plans) may be NULL, and so may purity, not both:
 *   *purity = sum over a, b of |rho[a, b]|^2,
 * a fixed-order fp64 sum over the finished matrix on the device (pieces of 4096 entries, a lane's 16 in ascending
 * order, a tree over the 256 lanes, the pieces likewise): with out == NULL the Renyi-2 entropy of a 4096-row cut needs
 * no 256 MiB download.  NOT normalised: the caller divides by (sum p)^2.
 * CTG_E_INVALID -- from one prologue, before anything is allocated or launched -- for a null exec, out and purity both
 * null, everything ctg_exec_result_marginal refuses, D > CTG_RDM_WIDE_MAX_DIM, and D <= CTG_RDM_MAX_DIM: that matrix is
 * ctg_exec_result_rdm's, one route per D, so its bits never depend on the entry that was called.
 *   - Exactly Hermitian: only b <= a is computed, the other half is written as its conjugate, Im rho[a, a] = 0.0.
 *   - Every product and sum is fp64 (v_mfma_f64_16x16x4_f64 on the power-of-two route); no floating-point atomics;
 *     every grid, split and association of a sum is a function of (dtype, extents, keep) alone.  The error bound per
 *     real component is that of ctg_exec_result_rdm.
 * ctg_rdm_wide_plan (host only, touches no device) returns what ctg_exec_result_rdm_wide launches for a result of
 * `dtype` (CTG_F32 .. CTG_C128) whose extents' product stands for result_elems, the same refusals included:
 *   words[0] route        0: power of two (every extent a power of two, at least 4096 elements), 1: general
 *   words[1] D
 *   words[2] edge         rows of a row panel: 64 (general: 1)
 *   words[3] panels       D / edge; row a is row a % edge of panel a / edge
 *   words[4] blocks       panels (panels + 1) / 2 of the lower triangle: block bi (bi + 1) / 2 + bj is panel bi x panel bj
 *   words[5] splits       along r: split s takes the chunks s * chunks / splits .. (s + 1) * chunks / splits - 1
 *   words[6] cols         values of r in a chunk (r row-major over the dropped axes): min(32, t); general: see below
 *   words[7] chunks       ceil(t / cols)
 *   words[8] grid         blocks * splits: workgroups of the tile kernel (general: work items, 256 to a workgroup)
 *   words[9] scratch      bytes of the executor's scratch the call lays out, at most CTG_RDM_WIDE_SCRATCH_BYTES(D)
 *   words[10] name        4 * route + dtype: "rdm_wide_kernel<T,64>" | "rdm_wide_general_kernel<T>", T in
 *                         float | double | c64 | c128
 * Power of two: workgroup (block, split) reads the one or two 64-row panels of its block chunk by chunk in ascending
 * order (16-byte loads, the next chunk's in flight), widens them to fp64 in LDS and keeps the block's 64 x 64 entries
 * in registers; a diagonal block computes its lower 16 x 16 tiles only.  splits doubles while blocks * splits < 512
 * and a split keeps at least 32 chunks; a finish kernel adds the splits' partials in ascending order and mirrors.
 * General: a serial walk per (pair a >= b, chunk of r), chunks of max(1024, ceil(t / 1024)) values, longer where the
 * per-chunk sums would pass 64 MiB; the chunks are added in ascending order; not tuned.
 * Scratch: the buffer of ctg_exec_result_topk (counted by ctg_exec_device_bytes, freed by ctg_exec_destroy): 16 D^2 bytes
 * for the matrix, 64 KiB of partials per (block, split) -- 8 D^2 + 512 D bytes when splits = 1, less than 64 MiB
 * otherwise -- and 8 bytes per 4096 entries for the purity: 387 MiB at D = 4096.  Not differentiable; no multi-rank
 * entry, as above. */
#define CTG_RDM_WIDE_MAX_DIM 4096
#define CTG_RDM_WIDE_PLAN_WORDS 11
#define CTG_RDM_WIDE_SCRATCH_BYTES(D)                                                                                  \
    (16ll * (D) * (D) + (8ll * (D) * (D) + 512ll * (D) > (64ll << 20) ? 8ll * (D) * (D) + 512ll * (D) : (64ll << 20)) + \
     (64ll << 10))
int ctg_exec_result_rdm_wide(ctg_exec* exec, int64_t rank, const int64_t* extents, const int32_t* keep, void* out,
                             double* purity);
int ctg_rdm_wide_plan(int32_t dtype, int64_t rank, const int64_t* extents, const int32_t* keep, int64_t* words);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION likewise (two new symbols; a binding that needs them looks them up):
 * the expectation values of ALL 2^L Pauli strings that share one X / Y pattern, by one Walsh-Hadamard transform on the
 * device (csrc/ctg_pauli_spectrum.hip) -- every <Z_i Z_j> and higher correlator, the Walsh
 * spectrum of an output distribution, all 4^k strings of a support (one call per X pattern).  extents[rank] is the shape
 * of the result x, n = 2^L elements: every extent must be 1 or 2.  flips[rank] in {0, 1} marks the axes that carry X or
 * Y (extent 2); xm is the mask of their flat-index bits (the flat bit of an axis is log2 of its row-major stride).  For
 * z in [0, n) the string P(xm, z) has Y on the bits of xm & z, X on xm & ~z, Z on z & ~xm, I elsewhere, and ny(z) =
 * popcount(xm & z) letters Y.  The spectrum is
 *   S[z] = <x| P(xm, z) |x>,
 * the value ctg_exec_result_pauli gives that string: NOT normalised, S[0] = sum p for xm = 0; row-major over the
 * tensor's own axes, Z / Y on the axes where the coordinate is 1.  With select == NULL the n doubles go to out (host, may
 * be NULL) and / or dev_out (device, 8-byte aligned, may be NULL; it must not overlap the result tensor); m is not read.
 * With select[m], m <= CTG_PAULI_SPECTRUM_MAX_SELECT entries in [0, n), out[s] = S[select[s]] (out must be given) and
 * dev_out, if given, still receives the whole spectrum.  The tensor is read as the calls above read it (whoever owns
 * the memory, the mantissa under strip_exponent, after the stream's earlier work, after the statistics passes, which
 * run first) and never written; the stream is synchronised.  CTG_E_NORM when sum p is not finite; an all-zero tensor
 * gives zeros.  CTG_E_INVALID -- checked on the host before anything is reserved or launched, all buffers untouched --
 * for everything ctg_exec_result_pauli refuses about exec, rank and extents, a null flips, an extent above 2, a flip
 * code above 1 or on an axis of extent 1, neither out nor dev_out, select without out, m out of range, a select entry
 * outside [0, n), a dev_out that is misaligned or overlaps the result tensor.  CTG_E_NOMEM when the scratch cannot be
 * reserved.
 *   - Arithmetic, all fp64, nothing contracted, associated as written: with p = x[j ^ xm], w = x[j],
 *       u[j] = (p.re w.re + p.im w.im) + (p.re w.im - p.im w.re)     (real plans: u[j] = p w),
 *     then for the bits b = 0, 1, .., L - 1 IN THIS ORDER every pair (a, c) = (v[j], v[j | 2^b]) becomes (a + c, a - c),
 *     then S[z] = (-1)^ceil(ny(z) / 2) v[z] by a flip of the sign bit; real plans: S[z] = +0.0 for odd ny(z).  (Re
 *     conj(p) w is symmetric under j <-> j ^ xm, Im conj(p) w antisymmetric: the part that does not belong to the parity
 *     of ny(z) cancels to rounding noise, so one real transform serves both parities.)
 *   - The bits of S are a function of (dtype, extents, flips, the tensor's bytes) alone: not of select, of which output
 *     was asked, earlier calls in the same scratch, or the executor.  No atomics.
 *   - |S[z] - exact| <= 2 (8 n + 1) 2^-53 sqrt(2) sum p for complex plans, 2 (n + 1) 2^-53 sum p for real plans.
 * ctg_pauli_spectrum_plan (host only, touches no device) returns what the call launches for a result of `dtype`
 * (CTG_F32 .. CTG_C128) whose extents' product stands for result_elems, the same refusals included:
 *   words[0] L
 *   words[1] xm
 *   words[2] partner      where x[j ^ xm] comes from -- 0: xm = 0, the element itself; 1: the thread's own 16-byte group;
 *                         2: another group of the same chunk of 4096 elements; 3: the chunk c ^ (xm >> 12).  Always a
 *                         second 16-byte load inside the tile pass: no separate form kernel runs.
 *   words[3] tile bits    min(L, 12): the bits "spectrum_tile_kernel<T>", T in float | double | c64 | c128, transforms
 *   words[4] passes       launches of "spectrum_pass_kernel": 0 for L <= 12, 1 for 13 .. 20, 2 for 21 .. 28, ...
 *   words[5 .. 8]         the bits of each pass, at most 8, ascending from bit 12
 *   words[9] tiles        workgroups of every launch: max(1, n / 4096)
 *   words[10] scratch     bytes of the vector in the executor's scratch when dev_out is not given (8 n, to 256); a
 *                         select table adds 8 m (to 256) twice: its copy and its values ("spectrum_gather_kernel")
 *   words[11] name        the dtype code: T of the tile kernel
 * Tile pass: 256 threads, two workgroups per CU, a workgroup per chunk of 4096 consecutive elements; u goes to 32 KiB of
 * LDS, the bits are transformed four at a time with 16 values per thread in registers.  Strided pass: in place, a
 * workgroup holds 2^bits rows of 4096 / 2^bits >= 16 consecutive doubles (runs of 128 bytes at least).  The last pass
 * applies the sign and the zeros.  Scratch: the buffer of ctg_exec_result_topk (counted by ctg_exec_device_bytes, freed
 * by ctg_exec_destroy).  Not differentiable; no multi-rank entry, as above. */
#define CTG_PAULI_SPECTRUM_MAX_SELECT (1 << 24)
#define CTG_PAULI_SPECTRUM_PLAN_WORDS 12
int ctg_exec_result_pauli_spectrum(ctg_exec* exec, int64_t rank, const int64_t* extents, const uint8_t* flips, int64_t m,
                                   const int64_t* select, double* out, void* dev_out);
int ctg_pauli_spectrum_plan(int32_t dtype, int64_t rank, const int64_t* extents, const uint8_t* flips, int64_t* words);
/* Added to ABI 10 WITHOUT a bump of CTG_ABI_VERSION likewise (two new symbols; a binding that needs them looks them up):
 * the distribution of a classical cost C(z) under p(z) = |x_z|^2 over the result tensor x, on the device
 * (csrc/ctg_cost.hip): conditional value at risk, quantiles, a histogram, moments, the optimum of C
 * over all n bitstrings and the probability of sampling it.  extents[rank] is the shape of x, n elements.
 * THE COST VECTOR C[0 .. n) (fp64) comes from exactly one of two sources.
 *   - Terms: ops[m][rank] with codes 0 (I) and 3 (Z) only (the rows of ctg_exec_result_pauli), coeffs[m] finite, m <=
 *     CTG_COST_MAX_TERMS; every extent must be 1 or 2 (n = 2^L).  C(z) = sum over s of coeffs[s] (-1)^popcount(z & m_s),
 *     m_s the flat-index mask of the Z axes of row s (the flat bit of an axis is log2 of its row-major stride): bit 1 of z
 *     means eigenvalue -1.  The host adds the coefficients of equal masks in ascending term order in fp64; the device
 *     zeroes the vector, stores each unique (mask, coefficient) pair and runs, for the bits b = 0, 1, .., L - 1 IN THIS
 *     ORDER, (a, c) = (v[j], v[j | 2^b]) -> (a + c, a - c), nothing contracted; every entry then gets + 0.0, so no -0.0
 *     survives.  The bits of C are a function of (extents, ops, coeffs) alone.
 *   - Values: dev_cost, n doubles on the device (8-byte aligned), any extents; never written.  A first pass refuses an
 *     entry that is not finite (CTG_E_INVALID, all outputs untouched).  -0.0 counts as +0.0.
 * INTEGER WEIGHTS.  S = sum p as ctg_exec_result_stats returns it = f 2^e, f in [1/2, 1); s = 62 - e (s = 0 for S = 0);
 * w_i = (uint64) rint(p_i 2^s): the scaling is exact, there is one rounding.  W = sum w < 2^63.  Every mass below is a
 * sum of w by 64-bit integer additions (order cannot matter; no floating-point atomics); divide by 2^s, and by S to
 * normalise.  An all-zero tensor: s = 0, W = 0, every mass 0, every level's A = 0 and t = +0.0, the support's extremes
 * 0.0 with index -1.  CTG_E_NORM when S is not finite.
 * LEVELS.  levels[nl], nl <= CTG_COST_MAX_LEVELS, each in (0, 1]; tail = -1 (lower) or +1 (upper).  A_l = ceil(alpha_l W)
 * exactly (alpha_l is a dyadic rational).  Lower tail: t_l = min{ c : sum over C(z) <= c of w_z >= A_l }, below_l = sum
 * over C(z) < t_l of w_z, at_l = sum over C(z) = t_l of w_z, tail_l = sum over C(z) < t_l of p_z C(z) (fp64).  The upper
 * tail is the same on -C, reported in C's own sign.  CVaR_l = (tail_l + (A_l - below_l) 2^-s t_l) / (A_l 2^-s).
 * HISTOGRAM.  edges[ne], ne = 0 or 2 <= ne <= CTG_COST_MAX_EDGES, finite, strictly ascending.  out_hist[ne + 1]:
 * out_hist[k] = sum of w_z over the z with k edges <= C(z), i.e. k = numpy's searchsorted(edges, C, "right"):
 * out_hist[0] the mass below the first edge, out_hist[ne] the mass at or above the last, out_hist[1 .. ne - 1] the bins.
 * out_words[CTG_COST_WORDS], each word an int64 (i) or the bits of a double (d):
 *   [0] s (i)   [1] W (i)   [2] sum p C (d)   [3] sum (p C) C (d)   [4] min C (d)  [5] its lowest flat index (i)
 *   [6] max C (d)  [7] its lowest index (i)   [8] min C over the support w > 0 (d)  [9] its lowest index (i)  [10] the
 *   mass at that value (i)   [11] max C over the support (d)  [12] index (i)  [13] mass (i)   [14] nl (i)  [15] tail (i)
 *   [16] S (d)   [17 .. 23] 0   [24 + 5 l ..]: A_l (i), t_l (d), below_l (i), at_l (i), tail_l (d)
 * fp64 sums (p C is one rounded product of SampleElem's p, (p C) C another) have a fixed association that depends on n
 * alone: a thread adds its 16 elements of a chunk of 4096 in index order, the wave by xor-butterflies, the four waves in
 * order, the chunks of a workgroup's contiguous span ascending, the spans ascending.  |sum - exact| <= (n + 5) 2^-53 sum
 * p |C|^k.
 * dev_cost_out, optional: n doubles on the device, 8-byte aligned, overlapping neither the result nor dev_cost; receives
 * C.  The call is synchronous; the tensor is read as the calls above read it and never written.  CTG_E_INVALID --
 * checked on the host before anything is reserved or launched, all outputs untouched -- for a null exec, extents or
 * out_words, what ctg_exec_result_pauli refuses about rank and extents, both sources or neither, ops without coeffs or
 * the reverse, a code other than 0 and 3, Z on an axis of extent 1, an extent above 2 with terms, m, nl or ne out of
 * range, a level outside (0, 1], edges not finite or not ascending, edges without out_hist, a coefficient that is not
 * finite (or whose absolute sum is not), a tail other than -1 and +1, a misaligned or overlapping dev_cost / dev_cost_out.
 * ctg_cost_plan (host only, touches no device) returns what the call launches for a result of `dtype` whose extents'
 * product stands for result_elems, source CTG_COST_TERMS or CTG_COST_VALUES, the same refusals included:
 *   words[0] L (values: -1)   [1] n   [2] tile bits min(L, 12) of "cost_tile_kernel"   [3] launches of "cost_pass_kernel"
 *   [4 .. 7] their bits   [8] workgroups of a transform launch   [9] digit passes per level: 6 (12, 12, 12, 12, 12, 4
 *   bits; without levels 1, which gives W)   [10] launches of "cost_digit_kernel<T>": 1 + 5 nl, each followed by
 *   "cost_rowsum_kernel" and "cost_select_kernel"   [11] workgroups of a digit pass and of "cost_final_kernel<T,H>"
 *   [12] scratch bytes with the vector in the scratch and no term table (16 bytes per unique mask more; 8 n less when
 *   dev_cost or dev_cost_out holds C)   [13] the dtype code   [14] chunks of 4096 elements   [15] histogram words ne + 1
 * Scratch: the buffer of ctg_exec_result_topk (counted by ctg_exec_device_bytes, freed by ctg_exec_destroy).  Not
 * differentiable; no multi-rank entry, as above. */
#define CTG_COST_MAX_TERMS (1 << 20)
#define CTG_COST_MAX_LEVELS 8
#define CTG_COST_MAX_EDGES 4097
#define CTG_COST_WORDS 64
#define CTG_COST_LEVEL_WORD0 24
#define CTG_COST_LEVEL_WORDS 5
#define CTG_COST_PLAN_WORDS 16
#define CTG_COST_TERMS 0
#define CTG_COST_VALUES 1
int ctg_exec_result_cost(ctg_exec* exec, int64_t rank, const int64_t* extents, int64_t m, const uint8_t* ops, const double* coeffs,
                         const void* dev_cost, int32_t tail, int64_t nl, const double* levels, int64_t ne, const double* edges,
                         int64_t* out_words, int64_t* out_hist, void* dev_cost_out);
int ctg_cost_plan(int32_t dtype, int64_t rank, const int64_t* extents, int32_t source, int64_t nl, int64_t ne, int64_t* words);
/* debugging aid: copy `n` elements of the arena starting at element `offset`
 * to the host (synchronous) */
int ctg_exec_download_arena(ctg_exec* exec, int64_t offset, int64_t n, void* host_out);

/* Checkpoint of a sliced run.  The reference sums slices into `result` one at
 * a time (`gather_slices`, core.py:3842-3844; `contract_mpi`, core.py:4073-4076),
 * so the whole state of an interrupted run is (slices done, partial sum[,
 * exponent]); which slices are done is the caller's cursor (it chose first /
 * count / stride).  `get_state` synchronises and copies the partial result
 * (result_elems elements) to the host together with the strip_exponent
 * exponent (0 / not-zero when stripping is off); `set_state` on a fresh
 * executor (same plan, same strip_exponent setting) replaces
 * ctg_exec_zero_result, after which run_slices continues the sum exactly where
 * it stopped: resuming is bit-identical to an uninterrupted run. */
int ctg_exec_get_state(ctg_exec* exec, void* host_result, double* exponent, int* zero);
int ctg_exec_set_state(ctg_exec* exec, const void* host_result, double exponent, int zero);
/* ABI 6.  Single-precision results (CTG_F32 / CTG_C64) of a sliced tree are summed in DOUBLE precision: the
 * executor keeps the running sum of the slices as CTG_F64 / CTG_C128 next to the result tensor, which always
 * holds that sum rounded once (a left fold of 2^20 slices in fp32 -- what the reference does, core.py:3842-3844
 * -- loses more than the 1e-5 this library promises); ctg_exec_reduce sums the ranks' double-precision sums.
 * The state of an interrupted run therefore is that sum: `ctg_exec_state_dtype` says in which element type
 * (the plan's own when there is no wider sum), `_wide` get / set move it (result_elems elements of that type);
 * the narrow pair above still works -- `ctg_exec_set_state` restarts the sum from the rounded values, which
 * is exact but not the bits an uninterrupted run would have carried. */
int ctg_exec_state_dtype(ctg_exec* exec, int* dtype);
int ctg_exec_get_state_wide(ctg_exec* exec, void* host_sum, double* exponent, int* zero);
int ctg_exec_set_state_wide(ctg_exec* exec, const void* host_sum, double exponent, int zero);

/* Multi-GPU: one process (or thread) per GPU, each with its own exec running
 * ctg_exec_run_share(exec, rank, world, 0, -1) -- ITS SHARE of the slices, dealt by the
 * library (ABI 6): the units rank, rank + world, ... where a unit is a whole slice group
 * (what a group shares is then computed once per group, on one rank) and a single slice
 * for a plan without group indices, which is the round-robin of `contract_mpi`
 * (core.py:4068-4076) -- followed by ONE collective over the result tensor: `comm.Allreduce` / `comm.Reduce` there (core.py:4081, 4089),
 * RCCL over xGMI here.  The communicator is created from a 128-byte unique id
 * made on one rank and handed to the others by whatever channel the caller has
 * (MPI bcast, a file, torch.distributed's store ...) -- the role of mpi4py's
 * COMM_WORLD in the reference (core.py:4057-4060).  RCCL is bound with dlopen
 * at the first call (librccl.so.1, librccl.so; CTG_RCCL_LIB names the one library to
 * bind instead -- no fallback when it cannot be loaded); CTG_E_COMM if it is absent. */
#define CTG_UNIQUE_ID_BYTES 128
int ctg_comm_get_unique_id(void* id_out /* [CTG_UNIQUE_ID_BYTES] */);
/* collective over all `world` ranks; `device` is this rank's GPU ordinal */
int ctg_comm_init(const void* id, int rank, int world, int device, ctg_comm** out);
int ctg_comm_info(const ctg_comm* comm, int* rank, int* world, int* device);
int ctg_comm_destroy(ctg_comm* comm);
/* Sum the ranks' result tensors in place, enqueued on the exec's stream behind
 * its slices: root < 0 -> every rank ends with the total (Allreduce,
 * core.py:4081); root >= 0 -> only `root` does, the others' result tensors are
 * left undefined (Reduce, core.py:4089).  With strip_exponent the partials are
 * (mantissa, exponent) pairs: the ranks first agree on the largest exponent,
 * rescale their mantissas to it (the adder of core.py:163-172 across ranks) and
 * then sum; ctg_exec_get_exponent returns the common exponent afterwards. */
int ctg_exec_reduce(ctg_exec* exec, ctg_comm* comm, int root);

/* Host-side tree tools (no GPU): the inner loops of path search and slicing.
 * The reference runs them in Python, or in its optional Rust accelerator
 * `cotengrust` when installed (pathfinders/path_basic.py:1351-1383); the
 * hyper-optimizers that call them stay in the reference unchanged.
 *
 * A network is given in CSR form: tensor t carries the index ids
 * inds[offsets[t] .. offsets[t+1]) (ids in [0, n_inds), repeats allowed),
 * `out_inds` are the output indices, `sizes[ix]` the extent of index ix. */

/* Greedy pairwise path (reference `optimize_greedy`, path_basic.py:616-700,
 * 1038-1106): score = size(ab)/costmod - (size(a)+size(b))*costmod, optional
 * Boltzmann sampling (temperature, seed), indices shared by more than
 * `max_neighbors` tensors generate no candidates (0 = no limit), disconnected
 * remainder combined smallest first.  Writes n_inputs-1 pairs of SSA ids
 * (inputs 0..n-1, intermediates n, n+1, ...) to ssa_path[2*(n_inputs-1)]. */
int ctg_path_greedy(int64_t n_inputs, const int64_t* offsets, const int64_t* inds, int64_t n_out,
                    const int64_t* out_inds, int64_t n_inds, const double* sizes, double costmod,
                    double temperature, int64_t max_neighbors, uint64_t seed, int64_t* ssa_path);

/* Greedy choice of indices to slice until the largest intermediate of the tree
 * `ssa_path` has at most 2^target_log2_size elements (reference `SliceFinder`
 * over `ContractionCosts`, slicer.py:17-201, 204-430; cost model: removing an
 * index of extent d divides the flops / sizes it takes part in by d and
 * multiplies the slice count by d).  Output indices are only used when
 * `allow_outer` (core.py:2632-2719).  Writes at most `max_sliced` index ids. */
int ctg_slice_greedy(int64_t n_inputs, const int64_t* offsets, const int64_t* inds, int64_t n_out,
                     const int64_t* out_inds, int64_t n_inds, const double* sizes,
                     const int64_t* ssa_path, double target_log2_size, int allow_outer,
                     int64_t max_sliced, int64_t* sliced, int64_t* n_sliced);

/* Subtree reconfiguration (reference `ContractionTree.subtree_reconfigure`,
 * core.py:2316-2449, with its dynamic-programming sub-optimizer): optimal
 * re-ordering of subtrees of `subtree_size` (2..16) leaves, most expensive node
 * first, at most `maxiter` subtree optimisations (<= 0: min(n_inputs, 1024)).
 * Cost of a contraction = flops + write_factor * size(result) -- the reference's
 * `combo-<write_factor>` objective (0: flops).  Give sliced indices size 1.
 * Reads ssa_path_in, writes ssa_path_out (both 2*(n_inputs-1) ids). */
int ctg_subtree_reconfigure(int64_t n_inputs, const int64_t* offsets, const int64_t* inds, int64_t n_out,
                            const int64_t* out_inds, int64_t n_inds, const double* sizes,
                            const int64_t* ssa_path_in, int64_t subtree_size, int64_t maxiter,
                            double write_factor, int64_t* ssa_path_out);

/* The same search with a machine model as the objective (no reference
 * counterpart; the reference's objectives are the `scoring.py` closed forms): a
 * contraction costs max(MACs / mac_rate_by_log2k[floor(log2 K)], (size_a + size_b
 * + size_out) / elem_rate) seconds, K = its contracted extent (the last table
 * entry serves every larger K), the MAC rate scaled by N/16 when the narrower
 * kept side has N < 16 columns and by 0.8 when it has 16..63 and K >= 64.  The table holds the caller's measurements of
 * the executor's kernels (cotengra_amd.pathfind.MI355X_C64). */
int ctg_subtree_reconfigure_timed(int64_t n_inputs, const int64_t* offsets, const int64_t* inds,
                                  int64_t n_out, const int64_t* out_inds, int64_t n_inds,
                                  const double* sizes, const int64_t* ssa_path_in, int64_t subtree_size,
                                  int64_t maxiter, const double* mac_rate_by_log2k, int64_t n_rates,
                                  double elem_rate, int64_t* ssa_path_out);

#ifdef __cplusplus
}
#endif
#endif /* CTG_HIP_H */
