// internal.hpp -- host-side interfaces between the translation units of libultragroth_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "dev_common.hpp"
#include "stream_timer.hpp"

namespace ug {

// ---- ntt.hip ------------------------------------------------------------------------------------------
Fr fr_root_of_unity(int s);
void bitrev_copy(u32* out, const u32* in, int logn, hipStream_t stream);

// Element-wise work folded into the first / last pass of a transform (the H-polynomial block's c = a o b and
// h = a o b - c, src/groth16.cpp:100-108,142-148) and a separate work buffer so that the inputs stay intact:
//   in2    first pass: the transform's input element is in[i] * in2[i]
//   work   intermediate passes run in place here (instead of on `in` / `out`)
//   fin_a, fin_b   last pass: out[i] = plain integer of fin_a[i] * fin_b[i] - x[i] (32-byte plain, not device form)
// The *_stride members matter only to a launch over several vectors (NttPlan::launch, vectors > 1): vector v of each buffer
// starts v * stride elements after the pointer.
struct NttFusion {
    const u32* in2 = nullptr; u32* work = nullptr; const u32* fin_a = nullptr; const u32* fin_b = nullptr;
    u64 in2_stride = 0, work_stride = 0, fin_a_stride = 0, fin_b_stride = 0;
};

// one pass of a transform as the host plans it (ntt.hip turns it into kernel arguments)
struct NttPass {
    const u32* in; u32* out; const u32* tw; const u32* post; const u32* post_const; const u32* in2; const u32* fin_a; const u32* fin_b;
    int logn, s0, k, j, gather_bitrev, scatter_bitrev;
    u64 in_stride, out_stride, in2_stride, fin_a_stride, fin_b_stride;      // elements between two vectors of each buffer (vectors > 1)
};
constexpr int NTT_MAX_PASSES = 8;

struct NttPlan {
    int logn = -1;
    DevBuf<u32> tw_fwd;       // stage-major twiddles omega_{2^(s+1)}^j (ntt.hip: 12-word Montgomery or 20-word Shoup entries)
    DevBuf<u32> tw_inv;       // omega_n^-i,  i < n/2
    DevBuf<u32> twist;        // n^-1 * omega_{2n}^i at place bitrev(i), i < n   (coset twist with the ifft scale folded in; in the
                              // order of the scattering pass that applies it)
    DevBuf<u32> ninv;         // n^-1 (one element)
    bool shoup = true;        // twiddle tables hold (w, floor(w 2^261 / q)) pairs and the butterflies make Shoup products (ntt.hip)
    void init(int logn, hipStream_t stream);
    void release();           // (ug_ctx_trim; the destructor needs no help)
    // DIT transform; see ntt.hip for the buffer rules. post / post_const are optional multipliers
    // applied in the last pass: out[i] *= post[i], or out[i] *= *post_const.
    // stats (optional): every pass launch is a timed section of it (stream_timer.hpp).
    // fuse (optional): see NttFusion.
    void transform(u32* out, const u32* in, bool inverse, bool gather_bitrev, bool scatter_bitrev,
                   const u32* post, const u32* post_const, hipStream_t stream, LaunchTimer stats = LaunchTimer(),
                   const struct NttFusion* fuse = nullptr, int vectors = 1, u64 out_stride = 0, u64 in_stride = 0) const;
    // the same in two steps, for callers that run several transforms of this size side by side: passes() fills `list`
    // (NTT_MAX_PASSES entries) and returns the pass count -- the same for every transform of the plan --, launch() runs pass
    // p of up to three such lists in one kernel launch (logn >= 1).
    // vectors > 1: the launch transforms `vectors` vectors per list (blockIdx.z), vector v of every data buffer v * its stride
    // (out_stride, in_stride, the fusion's) elements after the list's pointer; the twiddles, post and post_const are shared.
    // vectors = 1 is the launch of a single transform, the strides unread.
    int passes(NttPass* list, u32* out, const u32* in, bool inverse, bool gather_bitrev, bool scatter_bitrev,
               const u32* post, const u32* post_const, const struct NttFusion* fuse = nullptr, u64 out_stride = 0, u64 in_stride = 0) const;
    void launch(const NttPass* const* lists, int count, int p, hipStream_t stream, LaunchTimer stats = LaunchTimer(), int vectors = 1) const;
};

// Every allocation or release of a per-proof device buffer (schedules, MSM workspaces, the sort's tables) moves this counter: a
// captured launch sequence (ug_graph) holds raw pointers into those buffers and is only replayed while the counter stands where
// it stood when the capture ended.
uint64_t alloc_epoch();
void alloc_epoch_bump();
// (re)allocation of such a buffer (msm.hip, sort.hip)
template <class T> void epoch_alloc(DevBuf<T>& b, size_t n) { alloc_epoch_bump(); b.alloc(n); }
// ... and its release: a buffer that was never allocated moves nothing
template <class T> void epoch_free(DevBuf<T>& b) { if (b.get()) alloc_epoch_bump(); b.release(); }

// ---- msm.hip ------------------------------------------------------------------------------------------
// Bucket classes (many-device provers, DESIGN.md section 7: the witness products sharded by BUCKET instead of by base point).
// A schedule with classes keeps only the (scalar, window) digits whose bucket b = |digit| - 1 has its residue b mod Q,
// Q = 2^q_log, in [r0, r0 + cnt): one bucket set of 2^(c-1) / Q buckets per owned residue, local id b >> q_log. The ranks of
// a node own disjoint residue ranges of the SAME scalars and the SAME (whole) base tables, so a rank sorts, accumulates and
// reduces its share of the entries at the full problem's window width -- no extra window, a share of the buckets -- and the
// weights come back on the host: a digit of magnitude b + 1 = Q (k + 1) - (Q - 1 - r), k = b >> q_log, r = b mod Q, so the sum
// of a residue's set is Q * S1 - (Q - 1 - r) * S0 with S1 = sum (k + 1) B_k (what the running-sum reduction yields) and
// S0 = sum B_k (its running sum, emitted beside it).
// The lowest `specials` bucket ids of every window -- the digits 1 .. specials, which small witness values (bits, bytes,
// counters) fill with up to millions of entries: one residue's owner would get all of bucket 0 -- are not owned by residue
// but by SCALAR RANGE: the schedule keeps such a digit iff its scalar lies in [sp_lo, sp_hi) (local indices); they get
// bucket ids of their own behind the regular sets, and their weighted sum (sum (b + 1) X_b) is a third output.
struct BucketClasses {
    int q_log = 0;               // 0: no classes, the schedule owns every bucket
    u32 r0 = 0, cnt = 1;         // owned residues [r0, r0 + cnt) of Q = 2^q_log
    u32 specials = 0;            // bucket ids below this are owned by scalar range
    u32 sp_lo = 0, sp_hi = 0;    // ... the scalars [sp_lo, sp_hi) of the schedule
    bool on() const { return q_log > 0; }
};
constexpr u32 MSM_MAX_SPECIALS = 64;     // (one wave sums a window's special buckets)

// How a scalar's window digits become (bucket key, entry) pairs: the kernel argument of the digit-making kernels (sort.hip)
struct DigitPlan {
    u64 n; int c, windows; u32 buckets, sentinel; int tables;      // buckets: per set; sentinel = total_buckets(): the key of a digit that is not kept
    u64 set_map, table_map;                                        // window tables: digit w goes to bucket set w mod stride and reads
                                                                   // table w / stride -- 4-bit field w of each map (<= 16 windows)
    int q_log; u32 r0, cnt, specials, sp_lo, sp_hi, special_base;  // bucket classes (q_log = 0: none); special_base = first special bucket id
    // several scalar vectors (MsmGeometry::vectors > 1; read only by the kernels' vector instantiations): padded scalar i is
    // element j = i - v vec_count of vector v = i / vec_count (a multiply-high by vec_magic, no division), read at
    // (v vec_stride + j); its digits go to bucket sets v vec_sets + wset and its entries keep the index j
    u32 vec_count, vec_magic; int vec_shift; u32 vec_sets; u64 vec_stride;
};

struct MsmGeometry {
    u64 n = 0;          // number of scalars
    int c = 0;          // window bits
    int windows = 0;    // digits per scalar: ceil(255 / c)
    u32 buckets = 0;    // per bucket set: 2^(c-1), with classes 2^(c-1-q_log)
    bool tables = false;  // fixed-base window tables: digit j of scalar i multiplies 2^(c j) P_i, read from table j, so
                          // every digit of every window lands in ONE bucket set (no Horner, 1/windows of the reduction)
    int stride = 1;       // strided tables (tables mode): table j holds 2^(stride c j) P_i, T = ceil(windows / stride) of them; digit w
                          // goes to bucket set w mod stride and reads table w / stride, since d 2^(c w) P = 2^(c (w mod s)) (d T_(w / s)):
                          // `stride` bucket sets, a Horner of `stride` steps on the host. stride = 1: one set; stride = windows: one table
    BucketClasses cls;
    // Several scalar vectors over the same bases (batched proofs): `vectors` vectors of `n / vectors` scalars each, vector v at
    // scalar offset v * vec_stride. Vector v's digits go to bucket sets v * window_sets() + wset, so a product's result block
    // holds the window sets of every vector, one vector after the other, and the host makes one Horner per vector. n counts the
    // scalars of all vectors. (set_vectors after choose / choose_tables; no bucket classes.)
    int vectors = 1;
    u64 vec_stride = 0;
    static MsmGeometry choose(u64 n, int force_c = 0);
    static MsmGeometry choose_tables(u64 n, int c, int stride = 1);   // validates 1 <= stride <= windows
    static int table_window(u64 n);                                    // cost-model window width for the tables mode
    static int table_count(int c, int stride) { const int w = (255 + c - 1) / c; return (w + stride - 1) / stride; }
    void set_classes(const BucketClasses& k);                          // after choose / choose_tables (divides `buckets`)
    void set_vectors(int v, u64 stride);                               // after choose / choose_tables (n: the scalars per vector)
    u64 vector_count() const { return n / (u64)vectors; }
    int window_sets() const { return tables ? stride : windows; }      // Horner steps on the host
    int class_sets() const { return cls.on() ? (int)cls.cnt : 1; }
    int bucket_windows() const { return window_sets() * class_sets() * vectors; }  // bucket sets the reduction sees: set (w, j) = w * class_sets + j
                                                                                   // (vectors: set (v, w) = v * window_sets + w)
    u64 special_buckets() const { return cls.on() ? (u64)window_sets() * cls.specials : 0; }     // ids behind the regular sets
    u64 total_buckets() const { return (u64)bucket_windows() * buckets + special_buckets(); }
    // points of a product's result block: S1 per set; with classes also S0 per set and one weighted sum of the specials per window
    int result_points() const { return cls.on() ? 2 * bucket_windows() + (cls.specials ? window_sets() : 0) : bucket_windows(); }
    // entries this schedule is expected to keep (uniform digits): what the segment length is chosen for
    u64 expected_entries() const { return cls.on() ? ((n * (u64)windows) >> cls.q_log) * cls.cnt : n * (u64)windows; }
    DigitPlan digit_plan() const {
        DigitPlan d;
        d.n = n; d.c = c; d.windows = windows; d.buckets = buckets; d.sentinel = (u32)total_buckets(); d.tables = tables ? 1 : 0;
        d.set_map = 0; d.table_map = 0;
        if (tables)
            for (int w = 0; w < windows && w < 16; w++) { d.set_map |= (u64)(w % stride) << (4 * w); d.table_map |= (u64)(w / stride) << (4 * w); }
        d.q_log = cls.q_log; d.r0 = cls.r0; d.cnt = cls.on() ? cls.cnt : 1; d.specials = cls.on() ? cls.specials : 0;
        d.sp_lo = cls.sp_lo; d.sp_hi = cls.sp_hi; d.special_base = (u32)((u64)bucket_windows() * buckets);
        d.vec_count = (u32)vector_count(); d.vec_magic = 0; d.vec_shift = 0; d.vec_sets = (u32)window_sets(); d.vec_stride = vec_stride;
        if (vectors > 1) {     // i / vec_count = (mulhi(i, magic) + i) >> shift for every i < 2^32 (round-up reciprocal)
            int l = 0;
            while (((u64)1 << l) < (u64)d.vec_count) l++;
            d.vec_magic = (u32)((((u64)1 << 32) * (((u64)1 << l) - d.vec_count)) / d.vec_count + 1);
            d.vec_shift = l;
        }
        return d;
    }
};
constexpr int MSM_MAX_VECTORS = 16;                                   // scalar vectors of one schedule (batched proofs)
constexpr int TABLE_INDEX_BITS = 27;                                   // entry = index | table << 27 | sign << 31
constexpr int TABLE_MIN_C = 16, TABLE_MAX_C = 24;                      // <= 16 tables (4 bits), <= 2^23 buckets
// Modelled cost of one MSM of n scalars in mixed additions (msm.hip): classic windows (tables = false), or window tables of
// width c and the given stride
double msm_model_cost(u64 n, int c, bool tables, int stride = 1);

struct HeavyBucket { u32 bucket, first_seg, last_seg, pad; };  // a bucket cut into many segment pieces

// ---- sort.hip: the hand-written LSD radix partition that groups a schedule's pairs by bucket ------------------------
int radix_plan(int bits, int* shift, int* bins_log);          // passes; low bits first
// the unsorted pair form: keys / vals [w * n + i] = window w of scalar i (only for scalars of more than 16 windows, i.e. tiny MSMs)
void digit_pairs(const u32* scalars, const DigitPlan& plan, u32* keys, u32* vals, hipStream_t stream);
struct RadixSorter {
    DevBuf<u32> lookback;         // tiles x 256 status words of the pass in flight
    DevBuf<u32> small;            // 4 x 256 bin counts / starts, one tile counter per pass
    u64 tiles_cap = 0;
    void reserve(u64 n_pairs, int ipt_min);
    void release();
    // see sort.hip; returns which of the two buffer pairs holds the sorted pairs
    int sort(const u32* scalars, const MsmGeometry& geo, u32 sentinel, u64 n_pairs, int bits,
             u32* const buf_keys[2], u32* const buf_vals[2], u32* error_flag, hipStream_t stream, u32* n_valid_out = nullptr,
             bool* dropped_out = nullptr);
    ~RadixSorter() { release(); }      // (the release moves the epoch: the members' own destructors would not)
};

// Signed-digit decomposition of n scalars, grouped by (window, bucket): shared by every base set that
// is multiplied by the same scalars (A, B1, B2 and C all use the witness, src/groth16.cpp:55-64).
struct MsmSchedule {
    MsmGeometry geo;
    const u32* keys = nullptr;    // sorted bucket ids (sentinel = total_buckets at the end)
    const u32* vals = nullptr;    // sorted entries: scalar index | table << 27 | sign << 31
    const u32* tkeys = nullptr;   // lane-transposed copies of keys / vals (see msm.hip: transposed_index)
    const u32* tvals = nullptr;
    DevBuf<u32> bucket_start;     // per bucket: first entry
    DevBuf<u32> bucket_count;     // per bucket: number of entries
    DevBuf<u32> small_list;       // buckets cut into 2 .. 32 segment pieces (meta[4] of them), any order
    int log_seg = 0;              // entries per lane of the segmented accumulation = 2^log_seg ...
    int log_seg_tail = 0;         // ... and 2^log_seg_tail for the segments of the last eighth of the entries (msm.hip: SegMap)
    DevBuf<u32> heavy_list;       // device: HeavyBucket[heavy_cap]
    u32 heavy_cap = 0;
    DevBuf<u32> medium_list;      // device: HeavyBucket[heavy_cap] for buckets of FIX_MAX < pieces <= MEDIUM_MAX
    DevBuf<u32> heavy_offsets;    // device: first task of each heavy bucket (n_heavy + 1 entries)
    DevBuf<u32> meta;             // device: [n_heavy, n_valid, n_heavy_tasks, n_medium, n_small, ., ., sort failure flag] -- read by the
                                  // kernels; the flag travels to the host with every product's result block
    // workspace
    DevBuf<u32> keys_a, keys_b, vals_a, vals_b;
    DevBuf<uint8_t> sort_tmp; size_t sort_tmp_bytes = 0;       // (the library sort's scratch: UG_SORT=cub, kept for A/B runs)
    RadixSorter sorter;
    u64 capacity_n = 0; u64 capacity_buckets = 0;
    void reserve(const MsmGeometry& g);
    void build(const u32* scalars_dev, const MsmGeometry& g, hipStream_t stream);   // scalars: n x 32 B plain integers
    void release();
    ~MsmSchedule() { release(); }
};

struct MsmWorkspace {
    DevBuf<u32> bucket_pts;      // total_buckets XYZZ records
    DevBuf<u32> chunk_pts;       // reduction scratch
    DevBuf<u32> chunk_pts2;
    DevBuf<u32> slot_pts;        // two partial sums per segment of the accumulation
    DevBuf<u32> task_pts;        // partial sums of the heavy-bucket tasks
    size_t bucket_bytes = 0, chunk_bytes = 0, slot_bytes = 0, task_bytes = 0;
    void reserve(const MsmGeometry& g, bool g2, u64 n_segments, u32 n_heavy_tasks, int sets = 1);
    void release();
    ~MsmWorkspace() { release(); }
};

// An MSM whose kernels and result copy are queued on the stream; the window sums arrive in `host` (pinned memory,
// bucket_windows * PT_WORDS words) once the stream is synchronised. Several may be queued back to back: the stream
// orders their use of the shared workspace.
struct MsmPending {
    bool g2 = false;
    bool empty = true;           // nothing was queued: the sum is the point at infinity
    int c = 0, window_sets = 0, class_sets = 1;
    int vectors = 1;             // the block holds the window sets of `vectors` scalar vectors, one after the other
    BucketClasses cls;           // cls.on(): the block holds [S1 per set | S0 per set | specials per window] (MsmGeometry::result_points)
    u32* host = nullptr;
};
constexpr int MSM_G2_PT_WORDS = 72;                 // words of a G2 XYZZ point in a result block (msm.hip: G2Cfg)
constexpr size_t MSM_PENDING_WORDS = 128 * 72;      // room for the largest result block (<= 127 G2 points); the LAST word
                                                    // receives the schedule's failure flag (meta[7])
constexpr int MSM_QUEUE_DEPTH = 8;                  // products a context may hold queued before ug_ctx_collect (one pinned result block each)
constexpr int MSM_BATCH_WIDTH = 4;                  // products of one msm_enqueue call
// One call of msm_enqueue: `count` products over one schedule, product j the sum of scalar_i * bases[i + delta] over the schedule's
// scalars (local index i; `bases`: n_bases packed affine records in device Montgomery form, (0,0) = infinity; entries whose base
// index falls outside [0, n_bases) are skipped), its window sums going to `host`.
// group = 2 or 3: the `count` = group products of ONE interleaved array of group-point records -- bases (n_bases: records per window
// table) and delta are read from product 0 only, host from every product. G1 only.
struct MsmCall {
    struct Product { const u32* bases = nullptr; u64 n_bases = 0; int64_t delta = 0; u32* host = nullptr; };
    int count = 0;
    Product products[MSM_BATCH_WIDTH];
    int group = 0;
};
// phase: the whole call, or its two halves made one after the other with the same arguments -- the accumulation launches, and
// everything behind them (on a stream that is ordered behind the accumulation)
constexpr int MSM_PHASE_ALL = 0, MSM_PHASE_ACCUMULATE = 1, MSM_PHASE_TAIL = 2;
// queues the call's kernels and result copies: one accumulation launch per product (one in all for a group), the latency-bound
// tail kernels once for all of them; pend[j] describes product j's result block for msm_collect_*
// stats: every accumulation launch is a timed section of it (stream_timer.hpp: LaunchTimer; units = the entries the launch
// walks). A sample is never dropped: when 64 pairs are outstanding and none has finished, the timer's pool grows.
void msm_enqueue(bool g2, const MsmSchedule& s, MsmWorkspace& ws, const MsmCall& call, hipStream_t stream, LaunchTimer stats, MsmPending* pend,
                 int phase = MSM_PHASE_ALL);
// 64-byte records of one member set -> record (slot0 + i) * members + member of a group array
void interleave_points_g1(u32* dst, const u32* src, u64 n, int members, int member, u64 slot0, hipStream_t stream);
// (vector: which scalar vector's sum, below p.vectors)
G1XYZZ msm_collect_g1(const MsmPending& p, int vector = 0);
G2XYZZ msm_collect_g2(const MsmPending& p, int vector = 0);

// zkey affine records (reference Montgomery form, R = 2^256) -> device form, in place on the device
void convert_points_g1(u32* pts, u64 n, hipStream_t stream);
void convert_points_g2(u32* pts, u64 n, hipStream_t stream);

// pts = `tables` tables of n records, table 0 filled: table j = 2^(doublings j) * table 0 (fixed-base window tables: doublings =
// stride * c)
// (first, count: only the tables of the points [first, first + count) -- one piece of a deferred build; default: all of them)
void build_window_tables(bool g2, u32* pts, u64 n, int doublings, int tables, hipStream_t stream, u64 first = 0, u64 count = ~(u64)0);

// bench / test tooling: out[i] = (seed + i) * G as zkey-format records (device buffer); G given as a host record
void synth_points(bool g2, u32* out_dev, const u32* gen_record_host, u64 seed, u64 n, hipStream_t stream);

// ---- check.hip ----------------------------------------------------------------------------------------
// n RAW zkey records on the device (before convert_points_*): every bad one does atomicMin(*fault, (index0 + i) << 2 | reason),
// reason = the first of UG_POINT_UNREDUCED / _OFF_CURVE / _OFF_SUBGROUP (G2, level 2 only) it breaks. *fault starts as all ones.
void check_points(bool g2, const u32* pts, u64 n, u64 index0, int level, unsigned long long* fault, hipStream_t stream);
// The same rules, one answer per record: status[i] = UG_POINT_OK or the first rule record i of this launch breaks (device memory, n bytes).
void check_points_mask(bool g2, const u32* pts, u64 n, int level, uint8_t* status, hipStream_t stream);

// ---- hpoly.hip ----------------------------------------------------------------------------------------
struct CoefMatrix {
    u64 ncoefs = 0; u32 domain = 0; int logn = 0;
    DevBuf<u32> row_ptr;        // 2*domain + 1 offsets, rows = m * domain + c
    DevBuf<u32> sig;            // signal index per entry
    DevBuf<u32> val;            // packed coefficient per entry (device form, pre-scaled so that
                                //   mul(w_plain, val) = w * coef in device Montgomery form)
    // raw44: ncoefs packed 44-byte records {u32 m, u32 c, u32 s, 32-byte coef} already on the device
    // (src/groth16.hpp:41-49). Returns false when a record is out of range.
    bool build(const uint8_t* raw44_dev, u64 ncoefs, u32 domain, u32 nvars, hipStream_t stream);
    void release();
};

// a_br[bitrev(c)] = sum coef * w  over m = 0 rows, b_br likewise for m = 1 (device form, packed)
void coef_matvec(u32* a_br, u32* b_br, const CoefMatrix& m, const u32* wtns_dev, int mask, hipStream_t stream);   // mask bit 0: A rows, bit 1: B rows
// the same for `vectors` witnesses in one launch: witness v at wtns_dev + v * wtns_stride elements, its results at a_br / b_br +
// v * out_stride elements; every row's coefficients are read once per tile of MATVEC_VT witnesses. vectors = 1 is coef_matvec.
constexpr int MATVEC_VT = 4;
void coef_matvec_vectors(u32* a_br, u32* b_br, u64 out_stride, const CoefMatrix& m, const u32* wtns_dev, u64 wtns_stride, int vectors,
                         hipStream_t stream);
// out[i] = x[i] * y[i]
void fr_mul_pointwise(u32* out, const u32* x, const u32* y, u64 n, hipStream_t stream);
// h[i] = plain integer of (a[i] * b[i] - c[i])      (src/groth16.cpp:142-148)
void fr_h_final(u32* h, const u32* a, const u32* b, const u32* c, u64 n, hipStream_t stream);
// ... for `vectors` vectors in one launch: vector v of h at v * h_stride elements, of a, b and c at v * in_stride
void fr_h_final_vectors(u32* h, u64 h_stride, const u32* a, const u32* b, const u32* c, u64 in_stride, u64 n, int vectors, hipStream_t stream);
// element-wise format changes, n elements of 32 bytes
void fr_from_mont256(u32* out, const u32* in, u64 n, hipStream_t stream);
void fr_to_mont256(u32* out, const u32* in, u64 n, hipStream_t stream);
void f_op_mont256(int which, int op, u32* out, const u32* a, const u32* b, u64 n, hipStream_t stream);
void gather_elements(u32* out, const u32* src, const u32* index_dev, u64 n, u64 src_n, hipStream_t stream);
void scatter_elements(u32* dst, const u32* index_dev, const u32* values_dev, u64 n, u64 dst_n, hipStream_t stream);
// dst[w_idx[i]] = push[p_idx[i]] for i < n in order (last write wins); push = [table[0] | table[1 + chunks[j]], j < n_chunks |
// table[1..]]; all pointers on the device, indices already validated; last_scratch: one zeroed u32 per element of dst
// table_dev: 1 + 2 L elements, [0] = rand (plain) on entry; fills inv2 = 1/(i + rand) and prod = freq[i] * inv2[i] (plain)
void lookup_table(u32* table_dev, const u32* freq_dev, u64 L, hipStream_t stream);
void apply_lookup(u32* dst, u32* last_scratch, const u32* w_idx, const u32* p_idx, u64 n, const u32* chunks, u64 n_chunks,
                  const u32* table, hipStream_t stream);
// The vector forms (a batched proof): witness v's lists and table inside ONE staging buffer, at these offsets in u32 words
// (r_off: its challenge, 8 words; t_off: its table of 1 + 2 L elements; r_off and t_off multiples of 8).
struct LookupVec { u64 n, n_chunks, L, w_off, p_off, c_off, f_off, r_off, t_off; };
// fills every witness's table from its challenge and frequencies (table[0] = the challenge), one launch
void lookup_tables_vectors(u32* stage, const LookupVec* vec_dev, int vectors, u64 max_L, hipStream_t stream);
// apply_lookup for every witness, vector v of dst at v * stride elements; last_scratch: vectors * stride zeroed u32
void apply_lookup_vectors(u32* dst, u64 stride, u32* last_scratch, const u32* stage, const LookupVec* vec_dev, int vectors, u64 max_n,
                          hipStream_t stream);


// ---- r1cs.hip -----------------------------------------------------------------------------------------
// the three matrices A, B, C of an .r1cs on the device, each a CSR triple of CoefMatrix's form over `rows` constraints
// (val = coef * 2^522 packed); passed to the kernels by value
struct R1csDev {
    u32 rows = 0;
    const u32* row_ptr[3] = {nullptr, nullptr, nullptr};
    const u32* sig[3] = {nullptr, nullptr, nullptr};
    const u32* val[3] = {nullptr, nullptr, nullptr};
};
// n plain coefficients below r (32 bytes each, as the file has them) -> packed coef * 2^522, in place
void r1cs_convert_coefs(u32* val, u64 n, hipStream_t stream);
// queues the check of one witness (plain integers, n_wires elements): words[0] = failing constraints, words[1] = ~(lowest failing
// index), both zeroed first on the stream; mask: rows device bytes (0 holds, 1 fails) or null
void r1cs_check(const R1csDev& m, const u32* wtns, unsigned long long* words, uint8_t* mask, hipStream_t stream);
// the same for `vectors` witnesses in ONE launch, witness v at wtns + v * wstride words: its two words at words + 2 v (all zeroed
// first, one memset), its status bytes at mask + v * rows (or null). A lane takes one constraint for a group of R1CS_VT witnesses
// (r1cs_vectors_group: one witness alone is a group of one; UG_R1CS_VT = 1, 2 or 4 overrides). Four per lane compile without scratch
// too, but at one wave per SIMD, and are slower (profiles/registry_batch.txt).
constexpr int R1CS_VT = 2;
int r1cs_vectors_group(int vectors);
void r1cs_check_vectors(const R1csDev& m, const u32* wtns, u64 wstride, int vectors, unsigned long long* words, uint8_t* mask, hipStream_t stream);
// the values A.w, B.w, C.w of constraint k as canonical plain integers (24 device words), one lane
void r1cs_row_values(const R1csDev& m, const u32* wtns, u32 k, u32* out24, hipStream_t stream);
// the probe against a zkey's coefficient matrix over z (n_wires plain values): *word = the lowest failing 2 * row + matrix, or all ones
void r1cs_match(const R1csDev& m, const CoefMatrix& zk, u32 n_public, const u32* z, unsigned long long* word, hipStream_t stream);

// ---- zkey_verify.hip ----------------------------------------------------------------------------------
// The fold of a key check: one lane per row of the domain, rho (n_wires plain integers) in the witness's place, two sums per
// matrix -- wires 0 .. n_public and the others. out: eight vectors of `domain` canonical plain integers, a^pub, b^pub, c^pub,
// a^priv, b^priv, c^priv, a = a^pub + a^priv, b; rows m.rows + s, s <= n_public, carry rho_s mod r in a^pub and a, rows above
// them zeros. The caller vouches for m.rows + n_public + 1 <= domain and n_public < n_wires.
void r1cs_fold(const R1csDev& m, const u32* rho, u32 n_public, u32 domain, u32* out, hipStream_t stream);
// the same with a class byte per wire (0, 1 or 2) and three sums per matrix: eleven vectors (zkey_verify.hip)
void r1cs_fold_classes(const R1csDev& m, const u32* rho, const uint8_t* cls, u32 n_public, u32 domain, u32* out, hipStream_t stream);
// dst[i] = src[first + i * step] over `count` G1 records of 64 bytes (any form: the records are copied, not read)
void points_take_every(u32* dst, const u32* src, u64 first, u64 step, u64 count, hipStream_t stream);

}  // namespace ug
