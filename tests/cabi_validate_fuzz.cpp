// cabi_validate_fuzz.cpp -- the plan validator of the C ABI under the address and undefined-behaviour sanitizers, as a
// stand-alone program: its own main, linked against the library's objects (csrc/ctg_runtime.hip and csrc/ctg_lds_host.hip
// compiled with -fsanitize=address,undefined), so the sanitizer runtime comes from the executable itself.  Built and run
// by tests/test_cabi_validate_fuzz.py, which also writes its input.
//
//   cabi_validate_fuzz RANDOM_PER_PLAN SEED FILE...
//
// A FILE is one planner-written plan in the word layout of tests/golden/gen/make_cabi_plan.py (int64 words: header[10] =
// magic, dtype, n_inputs, inputs_elems, arena_elems, result_elems, n_steps, n_table_words, n_sliced, nslices; then
// input_sizes, input_offsets, steps, tables, slice_sizes, slice_fixed, slice_strides), followed by slice_group[n_sliced]
// and the mutation list of tests/test_plan_validation.py: n_mutants, then per mutant {expect (1 accept, 0 reject),
// n_edits, n_edits x {field, index, value}}; field codes are positions in that module's FIELDS.
//
// The program (1) creates the plan as it is, (2) replays the list -- a mutant judged otherwise than the list says ends
// the run --, (3) adds RANDOM_PER_PLAN seeded mutants of one to four words, the words drawn from the step records, the
// table blob and the descriptor's arrays, the values from the hostile values of every word class.  For every plan
// ctg_plan_create accepts it calls the plan queries and ctg_plan_host_reads_: every host function executor creation
// runs over a plan's tables before anything is uploaded (gather orders, vector tests, forms and packing of the LDS
// components).  It makes NO ctg_exec_* call and no HIP call: a mutated plan never reaches an executor.
// Exit status 0 and nothing from a sanitizer on stderr: the validator itself stayed inside its memory and inside 64 bits
// while it judged, and so did everything that trusts what it accepted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ctg_hip.h"

extern "C" int64_t ctg_plan_host_reads_(const ctg_plan* plan);   // (not part of the ABI: csrc/ctg_exec_state.h)

namespace {

constexpr int64_t kMagic = 0x43544750;
enum Field { F_INPUT_SIZES, F_INPUT_OFFSETS, F_STEPS, F_TABLES, F_SLICE_SIZES, F_SLICE_FIXED, F_SLICE_STRIDES, F_SLICE_GROUP,
             F_DTYPE, F_INPUTS_ELEMS, F_ARENA_ELEMS, F_RESULT_ELEMS, F_COUNT };

struct Plan {
    int64_t dtype, n_inputs, inputs_elems, arena_elems, result_elems, n_steps, n_table_words, n_sliced, nslices;
    std::vector<int64_t> arr[8];
};
struct Edit { int64_t field, index, value; };

uint64_t g_rng = 1;
uint64_t rnd() {   // xorshift64*
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

int64_t g_digest = 0, g_accepted = 0, g_rejected = 0;

// ctg_plan_create on `base` with `edits`; an accepted plan goes through every host-only reader, then is destroyed
int create(const Plan& base, const std::vector<Edit>& edits) {
    Plan p = base;
    for (const Edit& e : edits) {
        if (e.field < 8) p.arr[e.field][(size_t)e.index] = e.value;
        else if (e.field == F_DTYPE) p.dtype = e.value;
        else if (e.field == F_INPUTS_ELEMS) p.inputs_elems = e.value;
        else if (e.field == F_ARENA_ELEMS) p.arena_elems = e.value;
        else p.result_elems = e.value;
    }
    ctg_plan_desc d{};
    d.dtype = (int32_t)p.dtype;
    d.n_inputs = p.n_inputs;
    d.input_sizes = p.arr[F_INPUT_SIZES].data();
    d.input_offsets = p.arr[F_INPUT_OFFSETS].data();
    d.inputs_elems = p.inputs_elems;
    d.arena_elems = p.arena_elems;
    d.result_elems = p.result_elems;
    d.n_steps = p.n_steps;
    d.steps = p.arr[F_STEPS].data();
    d.n_table_words = p.n_table_words;
    d.tables = p.arr[F_TABLES].data();
    d.n_sliced = p.n_sliced;
    d.slice_sizes = p.arr[F_SLICE_SIZES].data();
    d.slice_fixed = p.arr[F_SLICE_FIXED].data();
    d.slice_strides = p.arr[F_SLICE_STRIDES].data();
    d.slice_group = p.arr[F_SLICE_GROUP].data();
    ctg_plan* h = nullptr;
    const int rc = ctg_plan_create(&d, &h);
    if (rc != CTG_OK) {
        ++g_rejected;
        return rc;
    }
    ++g_accepted;
    int64_t n = 0, ws[4] = {0, 0, 0, 0}, units = 0, per = 0;
    if (ctg_plan_nslices(h, &n) != CTG_OK || ctg_plan_workspace_bytes(h, ws) != CTG_OK ||
        ctg_plan_share_units(h, 0, 1, &units, &per) != CTG_OK) {
        fprintf(stderr, "a plan query failed on an accepted plan: %s\n", ctg_last_error());
        exit(3);
    }
    g_digest += n + ws[3] + units + per;
    for (int64_t s = 0; s < p.n_steps; ++s) {
        int ok = 0;
        if (ctg_plan_stem_pair16(h, s, &ok) == CTG_OK) g_digest += ok;
    }
    g_digest += ctg_plan_host_reads_(h);
    ctg_plan_destroy(h);
    return CTG_OK;
}

bool read_words(FILE* f, std::vector<int64_t>& v, int64_t n) {
    v.resize((size_t)n);
    return n == 0 || fread(v.data(), 8, (size_t)n, f) == (size_t)n;
}

// hostile values of every word class, for word `cur` of plan `p` (tests/plan_words.py: the classes)
int64_t hostile(const Plan& p, int64_t cur) {
    const int64_t caps[3] = {p.inputs_elems, p.arena_elems, p.result_elems};
    const int64_t cap = caps[rnd() % 3], blob = p.n_table_words;
    // (sums of the program's own are formed modulo 2^64: the sanitizer watches this file too)
    auto add = [](int64_t x, int64_t y) { return (int64_t)((uint64_t)x + (uint64_t)y); };
    const int64_t pool[] = {-1, -7, -2, 0, 1, 2, 3, 4, add(cur, 1), add(cur, -1), add(cur, cur), blob - 1, blob, blob + 1,
                            add(blob, -cur), cap - 1, cap, cap + 1, add(cap + 1, -cur), p.n_inputs + 1, p.n_steps, 65536,
                            1ll << 31, 1ll << 40, (1ll << 56) + 1, 1ll << 62, add(INT64_MAX, add(1, -cur)), INT64_MAX - 1,
                            INT64_MAX, INT64_MIN};
    return pool[rnd() % (sizeof(pool) / sizeof(pool[0]))];
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s RANDOM_PER_PLAN SEED FILE...\n", argv[0]);
        return 2;
    }
    const int64_t n_random = atoll(argv[1]);
    const uint64_t seed = strtoull(argv[2], nullptr, 10);
    int64_t replayed = 0, random_done = 0;
    for (int a = 3; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        std::vector<int64_t> head;
        if (!f || !read_words(f, head, 10) || head[0] != kMagic) {
            fprintf(stderr, "%s: not a plan file\n", argv[a]);
            return 2;
        }
        Plan p{head[1], head[2], head[3], head[4], head[5], head[6], head[7], head[8], head[9], {}};
        const int64_t lens[8] = {p.n_inputs, p.n_inputs, p.n_steps * CTG_STEP_WORDS, p.n_table_words, p.n_sliced, p.n_sliced,
                                 (p.n_inputs + 1) * p.n_sliced, p.n_sliced};
        // (file order: sizes, offsets, steps, tables, slice sizes, fixed, strides, then the group flags)
        for (int i = 0; i < 8; ++i)
            if (!read_words(f, p.arr[i], lens[i])) {
                fprintf(stderr, "%s: truncated\n", argv[a]);
                return 2;
            }
        if (create(p, {}) != CTG_OK) {
            fprintf(stderr, "%s: the planner's own plan is rejected: %s\n", argv[a], ctg_last_error());
            return 1;
        }
        // (2) the mutation list
        std::vector<int64_t> w;
        if (!read_words(f, w, 1)) return 2;
        const int64_t n_mut = w[0];
        for (int64_t m = 0; m < n_mut; ++m) {
            if (!read_words(f, w, 2)) return 2;
            const int64_t expect = w[0], n_edits = w[1];
            std::vector<Edit> edits((size_t)n_edits);
            for (Edit& e : edits) {
                if (!read_words(f, w, 3) || w[0] < 0 || w[0] >= F_COUNT || (w[0] < 8 && (w[1] < 0 || w[1] >= lens[w[0]]))) return 2;
                e = Edit{w[0], w[1], w[2]};
            }
            const int rc = create(p, edits);
            ++replayed;
            if ((expect == 1) != (rc == CTG_OK) || (rc != CTG_OK && rc != CTG_E_INVALID && rc != CTG_E_BOUNDS)) {
                fprintf(stderr, "%s: mutant %lld (field %lld index %lld value %lld): expected %s, got %d (%s)\n", argv[a],
                        (long long)m, (long long)edits[0].field, (long long)edits[0].index, (long long)edits[0].value,
                        expect ? "accept" : "reject", rc, rc ? ctg_last_error() : "");
                return 1;
            }
        }
        fclose(f);
        // (3) seeded random mutants: one to four words of the step records (half of them), the blob, the arrays
        g_rng = seed * 0x9E3779B97F4A7C15ull + (uint64_t)a;
        if (g_rng == 0) g_rng = 1;
        for (int64_t m = 0; m < n_random; ++m) {
            std::vector<Edit> edits(1 + rnd() % 4);
            for (Edit& e : edits) {
                const uint64_t pick = rnd() % 10;
                int64_t field = pick < 5 ? F_STEPS : (pick < 8 ? F_TABLES : (int64_t)(rnd() % F_COUNT));
                if (field < 8 && lens[field] == 0) field = F_STEPS;
                if (field < 8) {
                    const int64_t idx = (int64_t)(rnd() % (uint64_t)lens[field]);
                    e = Edit{field, idx, hostile(p, p.arr[field][(size_t)idx])};
                } else {
                    const int64_t cur = field == F_DTYPE ? p.dtype : (field == F_INPUTS_ELEMS ? p.inputs_elems
                                        : (field == F_ARENA_ELEMS ? p.arena_elems : p.result_elems));
                    e = Edit{field, 0, hostile(p, cur)};
                }
            }
            const int rc = create(p, edits);
            ++random_done;
            if (rc != CTG_OK && rc != CTG_E_INVALID && rc != CTG_E_BOUNDS) {
                fprintf(stderr, "%s: random mutant %lld: rc %d (%s)\n", argv[a], (long long)m, rc, ctg_last_error());
                return 1;
            }
        }
    }
    printf("replayed %lld listed and %lld random mutants: %lld accepted, %lld rejected (digest %lld)\n", (long long)replayed,
           (long long)random_done, (long long)g_accepted, (long long)g_rejected, (long long)g_digest);
    return 0;
}
