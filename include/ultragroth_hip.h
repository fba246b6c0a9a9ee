/*
 * ultragroth_hip.h -- inner C-ABI of libultragroth_hip.so: the MI355X (gfx950) replacement for the
 * arithmetic layer that rarimo/ultragroth's prover reaches through the un-vendored iden3/ffiasm
 * submodule. Plain pointers and sizes only; no exceptions cross this boundary (every function returns
 * UG_OK or UG_ERROR and ug_last_error() gives the message for the calling thread).
 *
 * Reference interface each group replaces (paths relative to the reference repository):
 *
 *   ug_bases_*  + ug_schedule_* + ug_msm_g1 / ug_msm_g2
 *       Curve::multiMulByScalarMSM(Point& r, PointAffine* bases, uint8_t* scalars, 32, n)
 *       call sites src/groth16.cpp:55,58,61,64,154 ; src/ultra_groth.cpp:168,201,214,227,234,322
 *       (the base arrays are the zkey sections handed to makeProver, src/groth16.cpp:9-46,
 *        src/prover.cpp:162-178)
 *
 *   ug_hpoly_create / ug_hpoly_run / ug_hpoly_run_vectors
 *       FFT<Fr>(2 * domainSize) ctor            src/groth16.hpp:109
 *       the a/b/c block of Prover::prove        src/groth16.cpp:66-148
 *         (zero, sparse coefficient scatter-add, a o b, 3 x {ifft, root(.) twist, fft}, a o b - c,
 *          fromMontgomery), twin in src/ultra_groth.cpp:243-320
 *
 *   ug_fr_ntt            FFT<Fr>::fft / ifft on a host buffer    (src/groth16.cpp:112,120)
 *   ug_field_op          F{r,q}_rawMMul / rawAdd / rawSub        (build/fr_raw_generic.cpp:11-39,107-148)
 *
 * Byte formats are the reference's: field elements are 32-byte little-endian; "Montgomery" means
 * value * 2^256 mod p (build/fr_raw_generic.cpp:192); G1 affine records are (x, y) Montgomery, 64 bytes;
 * G2 records are (x.a, x.b, y.a, y.b), 128 bytes; an all-zero record is the point at infinity; MSM
 * scalars and witness values are plain integers. Inputs may be unaligned (zkey sections start at
 * 4 mod 8); outputs are written with memcpy semantics.
 *
 * Environment variables read by libultragroth_hip.so (all optional; every setting of the first two groups gives correct
 * results):
 *
 *   deployment         ULTRAGROTH_DEVICE=n        device of a prover made by the reference's create calls (default 0)
 *                      ULTRAGROTH_DEVICES=a,b,..  one proof sharded over the listed devices behind the reference's API
 *                      ULTRAGROTH_VALIDATE=0|1|2  check every base point of a zkey on the device while a prover is created: 0 / unset
 *                                                 never (default) | 1 field range and curve equation | 2 also the G2 points'
 *                                                 membership of the order-r subgroup (include/prover.h: a bad key is refused)
 *                                                 (any other value fails the creation)
 *                      ULTRAGROTH_R1CS=<path>     every prover made by the reference's create calls attaches that .r1cs and checks the
 *                                                 witness of every proof against it (include/prover.h: ug_prover_attach_r1cs); an
 *                                                 unreadable or mismatching file, or a prover that cannot check, fails the creation
 *                                                 (unset / empty: nothing changes)
 *                      ULTRAGROTH_VERIFY_JUDGE=0|1  ug_groth16_verify_batch / ug_ultra_groth_verify_batch: 1 = the suspects of a rejected
 *                                                 batch are decided by their own equations on the device (include/verifier.h, the
 *                                                 judge; the same verdicts) | 0 / unset: searched and verified on the host (default)
 *                                                 (any other value fails the call)
 *                      ULTRAGROTH_TABLES=0|1|2    fixed-base window tables: never | created provers (default) | one-shot calls too
 *                      ULTRAGROTH_OVERLAP=0|1|2   H branch behind / beside (default since round 5) the witness products on one device
 *                                                 (0: one kernel on the chip at a time, for clean per-kernel times)
 *                      ULTRAGROTH_TABLES_BUDGET=g  the most HBM, in GiB, the window tables of a created prover may take (unset: the
 *                                                 free memory less the workspace reserve; 0 acts like ULTRAGROTH_TABLES=0). Below what
 *                                                 full tables take, ug_plan_window_tables picks strided tables or none per group
 *                      ULTRAGROTH_TABLES_BG=0     groth16_prover_create waits for its window tables (default: returns once the zkey is
 *                                                 resident; the tables are built in pieces between proofs, include/prover.h)
 *                      ULTRAGROTH_GRAPH=1         the device part of a created prover's proof recorded once per witness buffer and
 *                                                 replayed as a hipGraph (exact; measured a wash on this runtime, so off by default)
 *                      ULTRAGROTH_WITNESS_GATHER=0  ULTRAGROTH_DEVICES: a chain rank uploads the whole witness over its own PCIe link
 *                                                 (default: it collects the other ranks' slices from their HBM, peer copies)
 *                      ULTRAGROTH_SPARSE_B=0      keep B1 / B2 dense (default: when at most 3/4 of a circuit's B points are real, the prover
 *                                                 keeps only those, with a schedule of its own over their scalars: -15 % per proof at
 *                                                 2^24 with half of the B points at infinity, -26 % with three quarters)
 *                      ULTRAGROTH_BATCH_HPOLY=1   a batched proof runs the H-polynomial block of a device pass as ONE
 *                                                 ug_hpoly_run_vectors call, in launch groups as large as the memory left beside the
 *                                                 pass allows (0 / unset, the default: once per witness; the same proofs either way;
 *                                                 the FFT time of a pass falls 1.6-2.9x, the time per proof does not move, and 2^24
 *                                                 is unmeasured: profiles/batch_hpoly_ab.txt)
 *                      ULTRAGROTH_TAILS=split     the G1 and G2 tails of the witness products side by side on two streams (exact; a wash)
 *                      ULTRAGROTH_FUSED=0         A, B1, C as separate base sets instead of one interleaved group
 *                      ULTRAGROTH_SHARD=PxB       many-device layout: P base-point ranges x B bucket classes
 *                      ULTRAGROTH_MAX_RANGE=n     scalars per schedule (tests: the piecewise path without a 2^27 circuit)
 *                      ULTRAGROTH_UPLOAD_THREADS=n, ULTRAGROTH_H_PRIORITY=h|n|l, ULTRAGROTH_TRACE=1 (phase times on stderr)
 *   tuning knobs       UG_MSM_C, UG_TABLE_C       window width of the classic / table schedules (default: cost model)
 *                      UG_SEG_LANES_LOG, UG_SEG_TAPER   segment length of the accumulation (default 2^20 lanes, tapered end)
 *                      UG_REDUCE_G1_LOG, UG_REDUCE_G2_LOG   lanes the bucket reduction keeps busy (default 17, 16)
 *                      UG_UPLOAD_PRIORITY=l|n|h   stream class of the witness staging lanes (default l)
 *                      UG_NTT_SHOUP=0             Montgomery-form twiddle products in the NTT passes (default: Shoup form, ff.hpp mul_shoup)
 *                      UG_R1CS_VT=1|2|4           witnesses per lane of the batched witness check (default 2; 4 leaves one wave per SIMD)
 *                      UG_SETUP_WINDOW_G1, UG_SETUP_WINDOW_G2   window width (4 .. 16) of the development setup's generator tables
 *   test hooks         ULTRAGROTH_TEST_HOOKS=1 enables ug_test_set_blinding / ULTRAGROTH_TEST_BLINDING and ug_test_inject_fault;
 *                      without it those calls fail and the variables are ignored
 *   measurement        NOT in this library: UG_SORT=cub (library sort, links hipcub), UG_GROUP_FOLD_LOG (gathers folded into
 *                      cache: WRONG sums), UG_NTT_FUSE_STEPS (WRONG results), UG_SORT_IPT / _SPL / _DROP, UG_NTT_BATCH, UG_MATVEC_TILED exist only in the
 *                      -DUG_MEASURE build (`make -C ultragroth_amd/csrc MEASURE=1 measure` -> libultragroth_hip_measure.so,
 *                      loaded with ULTRAGROTH_LIB=<path> by the Python mirror); tests/test_abi.py checks that the product
 *                      library holds none of these names and no hipcub symbol.
 */
#ifndef ULTRAGROTH_HIP_H
#define ULTRAGROTH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UG_OK 0
#define UG_ERROR 1

#define UG_FIELD_FR 0
#define UG_FIELD_FQ 1
#define UG_OP_MUL 0
#define UG_OP_ADD 1
#define UG_OP_SUB 2
#define UG_OP_SQR 3

typedef struct ug_ctx ug_ctx;            /* one device + one stream + reusable workspaces           */
typedef struct ug_bases ug_bases;        /* a G1 or G2 base-point array resident in HBM              */
typedef struct ug_dvec ug_dvec;          /* a device vector of 32-byte elements (witness, h, ...)    */
typedef struct ug_index ug_index;        /* a list of 32-bit indices resident in HBM                  */
typedef struct ug_schedule ug_schedule;  /* signed-digit bucket schedule of a range of a ug_dvec     */
typedef struct ug_hpoly ug_hpoly;        /* coefficient matrix + NTT tables of one circuit           */

/* message of the last failing call on this thread ("" if none) */
const char* ug_last_error(void);
/* number of visible HIP devices, or -1 when the HIP runtime cannot be initialised */
int ug_device_count(void);

int  ug_ctx_create(ug_ctx** ctx, int device);
/* The same with a stream priority class: +1 = the device's highest, 0 = normal, -1 = its lowest (a tuning knob: on MI355X /
 * ROCm 7.2 two compute streams of different classes were measured to share the chip exactly as two of the same class do). */
int  ug_ctx_create_priority(ug_ctx** ctx, int device, int priority_class);
void ug_ctx_destroy(ug_ctx* ctx);
/* block until all work queued on the context's stream has finished */
int  ug_ctx_sync(ug_ctx* ctx);

/* Upload n affine points (zkey record format) and convert them to the device form. The array stands for
 * the global point indices [global_first, global_first + n) of its zkey section, so that a rank of a
 * sharded prover can hold a slice. */
int  ug_bases_create_g1(ug_ctx* ctx, const void* host_points, uint64_t n, uint64_t global_first, ug_bases** out);
int  ug_bases_create_g2(ug_ctx* ctx, const void* host_points, uint64_t n, uint64_t global_first, ug_bases** out);
/* The same WITH the fixed-base window tables described below (table_c = their window width, 0 = none): the tables are
 * allocated with the set, the points are uploaded straight into table 0 and the table kernel is queued on the context
 * without a host wait, so the upload of the caller's next section overlaps it (zkey ingest). Work queued
 * on the context afterwards is ordered behind the build; ug_ctx_sync waits for it. */
int  ug_bases_create_tables_g1(ug_ctx* ctx, const void* host_points, uint64_t n, uint64_t global_first, int table_c, ug_bases** out);
int  ug_bases_create_tables_g2(ug_ctx* ctx, const void* host_points, uint64_t n, uint64_t global_first, int table_c, ug_bases** out);
/* Fixed-base window tables (no reference counterpart: the zkey's points never change between proofs, and 288 GB of
 * HBM holds them): extend the set by tables 2^(c j) * P_i, j = 1 .. ceil(255/c) - 1, c in [16, 24]. A schedule built
 * with ug_schedule_build_tables(.., c) then puts every window digit into ONE bucket set. Fails (nothing changed)
 * when device memory is short. ug_msm_table_window: the cost-model width for n scalars; ug_bases_tables_bytes: the
 * additional device memory the tables take. */
int      ug_msm_table_window(uint64_t n);
uint64_t ug_bases_tables_bytes(uint64_t n, int g2, int c);
int      ug_bases_precompute(ug_bases* b, int c);
/* give the tables' memory back (the set keeps its n points; schedules must then be built without tables) */
int      ug_bases_drop_tables(ug_bases* b);
int      ug_bases_table_window(const ug_bases* b);          /* width of the tables held, 0 = none */
/* STRIDED TABLES: with stride s in [1, W], W = ceil(255/c), a set holds T = ceil(W/s) tables 2^(s c j) * P_i, j < T. A digit of
 * window w goes to bucket set w mod s and reads table w / s (d 2^(c w) P = 2^(c (w mod s)) (d T_(w/s))): s bucket sets per product,
 * combined on the host by a Horner of s steps. s = 1 is the plain table form above; s = W is one table (the points alone) at the
 * table-mode widths. A schedule of ug_schedule_build_tables_strided(.., c, s) needs bases of the same width AND stride, and no
 * bucket classes (they need one bucket set per product). ug_bases_tables_bytes_strided: the additional memory (T - 1) n records;
 * ug_bases_table_stride: the stride of the tables held, 0 = none. The plain calls are the s = 1 case. */
int      ug_bases_create_tables_strided_g1(ug_ctx* ctx, const void* host_points, uint64_t n, uint64_t global_first, int table_c, int stride,
                                           ug_bases** out);
int      ug_bases_create_tables_strided_g2(ug_ctx* ctx, const void* host_points, uint64_t n, uint64_t global_first, int table_c, int stride,
                                           ug_bases** out);
int      ug_bases_precompute_strided(ug_bases* b, int c, int stride);
uint64_t ug_bases_tables_bytes_strided(uint64_t n, int g2, int c, int stride);
int      ug_bases_table_stride(const ug_bases* b);
/* WINDOW-TABLE PLAN (host only, no device needed): one entry per group of base sets that share a schedule -- its scalars per
 * schedule and the points of its G1 and G2 sets. A group qualifies with 2^14 <= scalars <= 2^26. When full tables for every
 * qualifying group fit budget_bytes, every such group gets c = ug_msm_table_window(scalars), stride 1. Otherwise each group gets
 * none (c = 0, stride 0) or one (c, stride), the choice that minimises the summed modelled MSM cost (G2 products weighted by their
 * cost against G1) within the budget; scalars * W <= 2^30 and stride * 2^(c-1) <= 2^24 buckets per product hold for every
 * choice. bytes: the additional memory of the group's
 * tables. Deterministic; the sum of the bytes never exceeds the budget. */
typedef struct { uint64_t scalars, g1_points, g2_points; } ug_table_group;
typedef struct { int c, stride; uint64_t bytes; } ug_table_choice;
int      ug_plan_window_tables(const ug_table_group* groups, int n_groups, uint64_t budget_bytes, ug_table_choice* out);
/* BATCH PLAN (host only, no device needed): how many witnesses one device pass of a batched proof takes (ug_schedule_build_vectors).
 * One entry per schedule of the prover -- its scalars and its window tables (c = 0: classic windows; else width c, stride) --,
 * the circuit's signals and H domain, the free device bytes and the witnesses requested. Returns V with 1 <= V <=
 * min(requested, UG_BATCH_MAX): the largest V for which every schedule's V-vector form keeps V * scalars * ceil(255 / c) <= 2^30
 * pairs, fewer than 2^31 buckets and at most 127 bucket sets (one result block), and for which V witness and h vectors, V-fold
 * sort buffers (64 bytes per pair) and V-fold bucket arrays (732 bytes per bucket) fit free_bytes. Deterministic. 0 on bad
 * arguments. */
#define UG_BATCH_MAX 16
typedef struct { uint64_t scalars; int c, stride; } ug_batch_schedule;
int      ug_plan_proof_batch(const ug_batch_schedule* schedules, int n_schedules, uint64_t n_vars, uint64_t domain, uint64_t free_bytes,
                             int requested);
/* The same for a prover whose pass keeps aux_bytes_per_witness more device bytes per witness (UltraGroth: the gathered round /
 * final scalars and the lookup staging): V * aux_bytes_per_witness is added to the memory the V-fold buffers must fit. With
 * aux_bytes_per_witness = 0 it returns what ug_plan_proof_batch returns; more aux bytes never give a larger V. */
int      ug_plan_proof_batch_aux(const ug_batch_schedule* schedules, int n_schedules, uint64_t n_vars, uint64_t domain,
                                 uint64_t aux_bytes_per_witness, uint64_t free_bytes, int requested);
/* DEFERRED TABLE BUILDS (cold start of a created prover): after ug_ctx_defer_tables(ctx, 1) the sets made by
 * ug_bases_create_tables_* / ug_bases_create_group_g1 on this context hold their points only and remember the width: nothing
 * is queued, not even the tables' memory is allocated. ug_bases_tables_step(set, max_points, &remaining) builds the tables of the next max_points points on the
 * context's stream and waits for them: a bounded piece of device time that the caller puts between proofs. Until
 * ug_bases_tables_ready(set) returns 1 the set is a plain set (schedules without tables read table 0 only; products over a table
 * schedule fail). Why pieces and not one kernel on a side stream: a table kernel's workgroups live for 17-26 ms, and whenever a
 * proof's kernel ends they take the free compute units -- measured, the first proof beside such a build took 2.0 s instead of 0.17. */
int      ug_ctx_defer_tables(ug_ctx* ctx, int on);
/* the room for a deferred set's tables: _alloc is nothing but the device allocation (no stream touched: it may run beside proofs; a
 * first allocation of 36 GiB was seen to take 1.1 s); _adopt, when nothing is queued on the set's context, moves the points into
 * table 0 of the new array, swaps it in and frees the old one. Then the pieces: */
int      ug_bases_tables_alloc(ug_bases* b, void** mem);
int      ug_bases_tables_adopt(ug_bases* b, void* mem);
int      ug_bases_tables_step(ug_bases* b, uint64_t max_points, uint64_t* remaining);
int      ug_bases_tables_ready(const ug_bases* b);
int      ug_ctx_mem_info(ug_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);
void ug_bases_destroy(ug_bases* b);

/* POINT VALIDATION (check.hip). A zkey record is checked as it arrives, Montgomery R = 2^256, before anything reduces it. The
 * all-zero record is the point at infinity and passes; any other record breaks the FIRST of these rules that applies:
 *   UG_POINT_UNREDUCED      a coordinate (any of the four Fq components of a G2 point) is >= q as a raw 256-bit integer
 *   UG_POINT_OFF_CURVE      y^2 != x^3 + 3 (G1), y^2 != x^3 + 3/(9+u) over Fq2 (G2)
 *   UG_POINT_OFF_SUBGROUP   level 2, G2 only: [r]P is not the point at infinity (the twist has cofactor 2q - r) */
#define UG_POINT_OK 0
#define UG_POINT_UNREDUCED 1
#define UG_POINT_OFF_CURVE 2
#define UG_POINT_OFF_SUBGROUP 3
typedef struct { uint64_t index; int reason; } ug_point_fault;
/* n zkey-format records in HOST memory, staged through the context as an upload is; level 1 = rules 1-2, level 2 = also rule 3.
 * UG_OK when the check ran (out->reason = UG_POINT_OK: every point passed; else the LOWEST bad index and the first rule it
 * breaks); UG_ERROR only for bad arguments / device errors. Keeps nothing resident. */
int  ug_points_check(ug_ctx* ctx, int g2, const void* host_points, uint64_t n, int level, ug_point_fault* out);
/* The mask form: the same rules, order, record format and level, answered for EVERY record in one pass. reasons[i] (n bytes, host
 * memory) is UG_POINT_OK or the first rule record i breaks; the lowest i with a non-zero reason, and that reason, are what
 * ug_points_check reports for the same buffer. The records are staged in the same 64 MiB pieces, the status bytes downloaded
 * per piece. Batch verification uses it to drop every pi_b outside the subgroup with one call. */
int  ug_points_check_mask(ug_ctx* ctx, int g2, const void* host_points, uint64_t n, int level, uint8_t* reasons);
/* As ug_ctx_defer_tables: after ug_ctx_check_points(ctx, level), every ug_bases_create_* / ug_bases_create_group_* on this
 * context checks its records at that level (0 = off, the default), each upload chunk behind its own DMA and before its
 * conversion. A bad point fails the creation with UG_ERROR, ug_last_error() = "point <global index>: <reason text>" (global
 * index = global_first + position) or "member <m> point <index>: ..." for a group (index = first[m] + position), *out
 * untouched, every device byte of the half-made set freed and no table build started. The reason texts are
 * "coordinate not below the field modulus", "not on the curve", "not in the subgroup of order r". */
int  ug_ctx_check_points(ug_ctx* ctx, int level);
/* What the last ug_bases_create_* / ug_bases_create_group_* on this context found, as numbers (callers that translate the index
 * need not read the message): out->reason = UG_POINT_OK when that creation met no bad point (whatever else it may have failed
 * on), else the fault its message names; *member (may be NULL) = the group member, -1 for a plain set. */
int  ug_ctx_last_point_fault(const ug_ctx* ctx, int* member, ug_point_fault* out);
/* the fixed reason text of UG_POINT_UNREDUCED / _OFF_CURVE / _OFF_SUBGROUP ("" for anything else) */
const char* ug_point_reason_text(int reason);

/* device vectors of n 32-byte elements */
int  ug_dvec_create(ug_ctx* ctx, uint64_t n, ug_dvec** out);
int  ug_dvec_upload(ug_dvec* v, const void* host, uint64_t n);           /* host -> device, n <= capacity */
/* the same into elements [first, first + n); `via`: the context whose stream and staging buffers carry the copy (NULL =
 * the vector's own), so that two host threads can fill disjoint ranges of one vector at the same time */
int  ug_dvec_upload_range(ug_dvec* v, const void* host, uint64_t first, uint64_t n, ug_ctx* via);
/* the same as ug_dvec_upload for a vector NOTHING queued on the device refers to (the caller vouches for it): the copy
 * uses the staging streams only and does not wait for the context's stream -- the witness of the NEXT proof is staged this
 * way from a second host thread while the current proof runs (groth16_prover_prove from two threads on one prover) */
int  ug_dvec_upload_idle(ug_dvec* v, const void* host, uint64_t n);
int  ug_dvec_download(const ug_dvec* v, void* host, uint64_t first, uint64_t n);
/* out[i] = src[index[i]] for i < n (UltraGroth round / final witness gathers, src/ultra_groth.cpp:415-445) */
int  ug_dvec_gather(ug_dvec* out, const ug_dvec* src, const uint32_t* host_index, uint64_t n);
/* the same with the index list kept on the device (the two lists are part of the zkey: upload once at create) */
int  ug_index_create(ug_ctx* ctx, const uint32_t* host_index, uint64_t n, ug_index** out);
void ug_index_destroy(ug_index* index);
int  ug_dvec_gather_index(ug_dvec* out, const ug_dvec* src, const ug_index* index);
/* the same into out[out_first, out_first + index size): vector v of a batched sparse-B schedule at v * its vector stride */
int  ug_dvec_gather_index_at(ug_dvec* out, uint64_t out_first, const ug_dvec* src, const ug_index* index);
/* dst[index[i]] = values[i] for i < n; indices must be distinct (UltraGroth lookup signals written back into the
 * witness, src/ultra_groth.cpp:99-105) */
int  ug_dvec_scatter(ug_dvec* dst, const uint32_t* host_index, const void* host_values, uint64_t n);
/* UltraGroth lookup completion (the loop of compute_lookup, src/ultra_groth.cpp:99-105, with its push_vector :62-98
 * left implicit): for i < n in order  dst[w_idx[i]] = push[p_idx[i]],  where
 *   push = [ table[0] | table[1 + chunks[j]] for j < n_chunks | table[1], ..., table[2 L] ],
 * table = [challenge | inv2[0..L) | prod[0..L)] as plain 32-byte integers (L = lookup_size). Writes to one index keep
 * the last. All arrays are host arrays; indices out of range fail with nothing written. */
int  ug_dvec_apply_lookup(ug_dvec* dst, const uint32_t* w_idx, const uint32_t* p_idx, uint64_t n,
                          const uint32_t* chunks, uint64_t n_chunks, const void* table, uint64_t lookup_size);
/* The lookup table of compute_lookup (src/ultra_groth.cpp:71-80) for challenge `rand_plain` (32-byte plain integer):
 * table_out = [rand | inv2[0..L) | prod[0..L)] with inv2[i] = 1 / (i + rand) (0 when i + rand = 0) and
 * prod[i] = frequencies[i] * inv2[i], plain integers, (1 + 2 L) * 32 bytes of host memory -- the `table` argument of
 * ug_dvec_apply_lookup. Row index and frequency follow the reference's (int, Element) overloads (>= 2^31: value - 2^32). */
int  ug_fr_lookup_table(ug_ctx* ctx, const void* rand_plain, const uint32_t* frequencies, uint64_t lookup_size, void* table_out);
/* VECTOR FORMS of the two calls above: the lookup completion of the V witnesses of a batched proof (1 <= V <= UG_BATCH_MAX),
 * whose lists may differ in content and length. lists[v] = the host arrays of witness v; vector v of dst is dst[v * vector_stride,
 * (v + 1) * vector_stride) and every w_idx of witness v must lie below vector_stride. Each call makes ONE staged upload of the
 * concatenated lists, one launch per kernel over all vectors, and ends with one host wait. "Last write wins" holds within each
 * witness as in ug_dvec_apply_lookup; the scratch that decides it is per vector. At V = 1 the results are byte-identical to the
 * single calls. Indices out of range fail the whole call with nothing written (the messages of ug_dvec_apply_lookup).
 *   ug_fr_lookup_tables            tables_out[v] = the table of (rands_plain + 32 v, lists[v].frequencies), (1 + 2 L_v) * 32 bytes;
 *                                  only frequencies / lookup_size of the lists are read
 *   ug_dvec_apply_lookup_vectors   the writes of every witness with host tables[v] (frequencies are not read)
 *   ug_dvec_complete_lookup_vectors  both in one call: the tables are made on the device, used there, and copied to
 *                                  tables_out[v] (may be NULL: not copied) -- still one upload and one host wait
 * ug_lookup_vectors_bytes: the device bytes such a call takes for these lists (staging and the per-vector scratch). */
typedef struct {
    const uint32_t* frequencies; uint64_t lookup_size;
    const uint32_t* chunks; uint64_t n_chunks;
    const uint32_t *w_idx, *p_idx; uint64_t n;
} ug_lookup_lists;
int  ug_fr_lookup_tables(ug_ctx* ctx, int vectors, const void* rands_plain, const ug_lookup_lists* lists, void* const* tables_out);
int  ug_dvec_apply_lookup_vectors(ug_dvec* dst, uint64_t vector_stride, int vectors, const ug_lookup_lists* lists, const void* const* tables);
int  ug_dvec_complete_lookup_vectors(ug_dvec* dst, uint64_t vector_stride, int vectors, const void* rands_plain,
                                     const ug_lookup_lists* lists, void* const* tables_out);
uint64_t ug_lookup_vectors_bytes(uint64_t vector_stride, const ug_lookup_lists* lists, int vectors);
/* non-owning view of n 32-byte elements already in device memory (e.g. a torch / RCCL buffer) */
int  ug_dvec_wrap(ug_ctx* ctx, void* device_ptr, uint64_t n, ug_dvec** out);
uint64_t ug_dvec_size(const ug_dvec* v);
/* raw device address of a vector's first element (for the phase calls of include/prover.h that take device pointers) */
void* ug_dvec_device_ptr(const ug_dvec* v);
/* dst[dst_first .. + count) = src[src_first .. + count) between vectors of ANY two devices of the node (blocking) */
int  ug_dvec_copy(ug_dvec* dst, uint64_t dst_first, const ug_dvec* src, uint64_t src_first, uint64_t count);
/* the same with the copy queued on `via`'s stream (a context of dst's device; NULL = dst's own) */
int  ug_dvec_copy_via(ug_dvec* dst, uint64_t dst_first, const ug_dvec* src, uint64_t src_first, uint64_t count, ug_ctx* via);
void ug_dvec_destroy(ug_dvec* v);

/* Decompose scalars [first, first + count) of `scalars` (plain 32-byte integers) into signed window
 * digits grouped by bucket. One schedule serves every base set multiplied by the same scalars. */
int  ug_schedule_create(ug_ctx* ctx, ug_schedule** out);
/* release the device buffers of a schedule / of a context's MSM workspaces (they are re-allocated by the next build /
 * product): what a resident multi-circuit prover trims first when HBM is short */
int  ug_schedule_trim(ug_schedule* s);
int  ug_ctx_trim(ug_ctx* ctx);
int  ug_schedule_build(ug_schedule* s, const ug_dvec* scalars, uint64_t first, uint64_t count);
/* the same for base sets that hold window tables of width c (ug_bases_precompute); count <= 2^27 */
int  ug_schedule_build_tables(ug_schedule* s, const ug_dvec* scalars, uint64_t first, uint64_t count, int c);
/* ... for strided tables of width c and stride s (ug_bases_create_tables_strided_g1) */
int  ug_schedule_build_tables_strided(ug_schedule* s, const ug_dvec* scalars, uint64_t first, uint64_t count, int c, int stride);
/* SEVERAL SCALAR VECTORS in one schedule (batched proofs: the witnesses of several proofs multiply the same bases): `vectors`
 * (1 .. 16) vectors of `count` scalars each, vector v at scalars [first + v * vector_stride, .. + count), vector_stride >= count;
 * every vector stands for the same global indices [first, first + count). table_c = 0: classic windows; otherwise window tables
 * of width table_c and stride `stride`. vectors = 1 is exactly ug_schedule_build / ug_schedule_build_tables_strided. Vector v's
 * digits go to bucket sets of its own, so ONE sort, one accumulation launch per product and one set of tails serve all of them.
 * Every product over such a schedule -- ug_msm_g1 / _g2, ug_msm_batch, ug_msm_batch_enqueue, ug_msm_group_enqueue,
 * ug_msm_witness_enqueue -- writes `vectors` CONSECUTIVE records into each of its outputs, record v = the product over vector v
 * (64 bytes each for G1, 128 for G2). Limits (the call fails otherwise): vectors * count * ceil(255 / c) <= 2^30 digits, fewer
 * than 2^31 buckets over all vectors, and at most 127 bucket sets over all vectors (classic windows: vectors * windows). No
 * bucket classes (ug_schedule_set_classes). ug_plan_proof_batch sizes V for a prover. */
int  ug_schedule_build_vectors(ug_schedule* s, const ug_dvec* scalars, uint64_t first, uint64_t count, int vectors, uint64_t vector_stride,
                               int table_c, int stride);
/* BUCKET CLASSES (a many-device prover that shards the witness products by bucket instead of by base point; DESIGN.md section 7,
 * no counterpart in the reference): every later build of the schedule keeps only the (scalar, window) digits whose bucket
 * b = |digit| - 1 has b mod 2^q_log in [first_residue, first_residue + residues) -- except the lowest `specials` (<= 64) bucket ids
 * of every window, the digits small witness values pile up in: those are kept iff their scalar's index (in the scalar vector) lies in
 * [special_first, special_first + special_count). Schedules built over the SAME scalars and base sets whose residue ranges tile
 * [0, 2^q_log) and whose special ranges tile the scalars give products that ADD UP to the product of the plain schedule: each
 * holds its share of the entries at the plain schedule's window width and reduces only its share of the buckets. q_log = 0
 * switches the classes off. Needs a window of at least q_log + 4 bits (ug_schedule_build* fail otherwise). */
int  ug_schedule_set_classes(ug_schedule* s, int q_log, uint32_t first_residue, uint32_t residues, uint32_t specials,
                             uint64_t special_first, uint64_t special_count);
void ug_schedule_destroy(ug_schedule* s);

/* out = sum over the schedule's scalars s_i (global index i) of s_i * P_{i - index_shift}; points whose
 * global index falls outside the uploaded slice are skipped. out is an affine record in the reference
 * format (64 bytes for G1, 128 for G2; all zero = infinity). */
int  ug_msm_g1(ug_ctx* ctx, const ug_bases* bases, const ug_schedule* s, int64_t index_shift, void* out_affine);
int  ug_msm_g2(ug_ctx* ctx, const ug_bases* bases, const ug_schedule* s, int64_t index_shift, void* out_affine);
/* count <= 8 products over ONE schedule (G1 and G2 sets mixed freely; index_shifts may be NULL), queued back to back with
 * a single host synchronisation: outs[k] receives what ug_msm_g1 / ug_msm_g2 would write for bases[k]. */
int  ug_msm_batch(ug_ctx* ctx, int count, const ug_bases* const* bases, const ug_schedule* s, const int64_t* index_shifts,
                  void* const* outs_affine);
/* The same in two halves, so that a whole proof needs ONE host wait: ug_msm_batch_enqueue queues the products (up to 8
 * per context may be pending; `outs` must stay valid) and returns at once; ug_ctx_collect waits for everything queued on
 * the context, then finishes the queued results on the host (Horner, affine conversion) into their `outs`. Schedules
 * (ug_schedule_build*) and ug_hpoly_run queue their work without a host wait as well. ug_ctx_wait orders two contexts on
 * the device: what is queued on `waiter` afterwards starts when what was queued on `signal` before has finished. */
int  ug_msm_batch_enqueue(ug_ctx* ctx, int count, const ug_bases* const* bases, const ug_schedule* schedule,
                          const int64_t* index_shifts, void* const* outs);
/* A GROUP of 2 or 3 G1 base sets that are always multiplied by the same scalars -- A, B1 and C of a Groth16 proof
 * (src/groth16.cpp:55,58,64 all read the witness; C with its index shift), A and B1 of an UltraGroth one -- kept as ONE array
 * of K-point records, so that the accumulation kernel reads the entry list once and gathers the K points of an entry from
 * adjacent memory. Member m brings n[m] points (zkey format), the first of which belongs to the scalar with global index
 * first[m]; the group covers scalars [group_first, group_first + slots), a slot a member has no point for is infinity.
 * table_c != 0: with fixed-base window tables of that width (as ug_bases_create_tables_g1). ug_msm_group_enqueue queues the K
 * products over a schedule (results in outs[m], 64 bytes each, after ug_ctx_collect); the schedule's range must lie in the
 * group's. ug_bases_destroy / _precompute / _drop_tables / _table_window accept a group. */
int  ug_bases_create_group_g1(ug_ctx* ctx, int members, const void* const* host_points, const uint64_t* n, const uint64_t* first,
                              uint64_t group_first, uint64_t slots, int table_c, ug_bases** out);
/* ... with strided tables (stride in [1, ceil(255 / table_c)]) */
int  ug_bases_create_group_strided_g1(ug_ctx* ctx, int members, const void* const* host_points, const uint64_t* n, const uint64_t* first,
                                      uint64_t group_first, uint64_t slots, int table_c, int stride, ug_bases** out);
int  ug_bases_members(const ug_bases* bases);
/* 1 when every one of the n records of `record_bytes` bytes at host_points is the point at infinity (all zero): such a set's products
 * are the point at infinity, no kernel runs for them (ug_bases_create_* mark the set themselves), and a prover keeps it out of a
 * base group. Stops at the first other record, i.e. at once for any real section. */
int  ug_points_all_infinity(const void* host_points, uint64_t n, uint64_t record_bytes);
int  ug_msm_group_enqueue(ug_ctx* ctx, const ug_bases* group, const ug_schedule* schedule, void* const* outs);
/* The witness products of a proof in one call -- the K products of a base group and ONE G2 set over the same schedule (S1-S4,
 * src/groth16.cpp:55-64): both accumulations back to back, then the G1 and the G2 tails (cut buckets, bucket reduction, tree sums,
 * result copies: chains of dependent EC additions) side by side on two streams. Results as after ug_msm_group_enqueue +
 * ug_msm_batch_enqueue: outs_group[m] (64 bytes each) and out_g2 (128 bytes) after ug_ctx_collect. */
int  ug_msm_witness_enqueue(ug_ctx* ctx, const ug_bases* group, const ug_bases* g2set, const ug_schedule* schedule,
                            void* const* outs_group, void* out_g2);
int  ug_ctx_collect(ug_ctx* ctx);
int  ug_ctx_wait(ug_ctx* waiter, ug_ctx* signal);
/* For a caller that queued work and then failed before ug_ctx_collect: waits for what is still running on the context (the
 * kernels read the caller's buffers) and forgets the queued products, whose `outs` may no longer exist. Never fails. */
void ug_ctx_abandon(ug_ctx* ctx);
/* Test hook, honoured only in processes started with ULTRAGROTH_TEST_HOOKS=1 (UG_ERROR otherwise): the `after`-th next call
 * that passes fault point `site` fails with "injected fault". Lets the tests take the error paths of a running proof. */
/* diagnostic: the passes (return value, <= 4; -1 on bad arguments) the schedule sort makes for keys below 2^bits, with the
 * bit offset and width of each pass's digit (csrc/sort.hip). Host arithmetic only. */
int  ug_sort_plan(int bits, int shift[4], int bins_log[4]);
#define UG_FAULT_HPOLY_RUN 1
#define UG_FAULT_SCHEDULE_BUILD 2
#define UG_FAULT_HPOLY_RESERVE 3       /* ug_hpoly_reserve_vectors, with three of the five new workspaces allocated */
int  ug_test_inject_fault(int site, int after);

/* coefs: n_coefs packed 44-byte records {u32 m, u32 c, u32 s, Fr coef} (zkey section 4 past its 4-byte
 * count, src/groth16.cpp:38). Builds the row-sorted matrix and the NTT tables for domain_size. */
int  ug_hpoly_create(ug_ctx* ctx, const void* host_coefs, uint64_t n_coefs, uint32_t domain_size,
                     uint32_t n_vars, ug_hpoly** out);
/* h (domain_size plain integers) from the witness (n_vars plain integers), all on the device */
int  ug_hpoly_run(ug_hpoly* hp, const ug_dvec* witness, ug_dvec* h_out);
/* The block for `vectors` witnesses in one call (1 <= vectors <= UG_BATCH_MAX; the V witnesses of a batched proof): vector v reads
 * witness[v * witness_stride, + n_vars) and writes h_out[v * h_stride, + domain_size) -- byte for byte what ug_hpoly_run writes for
 * that witness -- and nothing else of h_out (the gaps of a strided h_out keep their contents; as in the single call, a vector's h
 * slice may serve as a work buffer before its result lands there). The vectors go in launch groups of the reserved size (the last
 * one may be smaller): a group's matrix-vector products are ONE launch that reads every coefficient once per four witnesses, and
 * each of its NTT passes is ONE launch over all its vectors. ug_hpoly_reserve_vectors gives the handle workspaces for `group`
 * vectors side by side, ug_hpoly_vectors_bytes(domain_size, group) bytes = group * 5 * 32 * domain_size; a created handle has
 * group 1 (run_vectors is then a loop of single-witness launches, and vectors = 1 queues exactly what ug_hpoly_run queues). A
 * reservation waits for the context's stream. A larger one allocates before it frees: if it does not fit it fails with UG_ERROR
 * and leaves the old one in use. A smaller one frees first, so that giving memory back never needs memory.
 * ug_hpoly_group: the largest launch group of the last ug_hpoly_run_vectors call, min(vectors, reserved group) (before any such
 * call: the reserved group). UG_ERROR with the reason in ug_last_error for: vectors outside 1 .. UG_BATCH_MAX, witness_stride <
 * n_vars, h_stride < domain_size, a vector shorter than its last slice. No host wait; may be recorded (ug_graph_begin). The
 * fault site UG_FAULT_HPOLY_RUN is passed once per witness. */
int      ug_hpoly_run_vectors(ug_hpoly* hp, const ug_dvec* witness, uint64_t witness_stride, int vectors,
                              ug_dvec* h_out, uint64_t h_stride);
int      ug_hpoly_reserve_vectors(ug_hpoly* hp, int group);   /* workspaces for `group` vectors side by side; 1..UG_BATCH_MAX */
int      ug_hpoly_group(const ug_hpoly* hp);                  /* vectors per launch group that the last run_vectors call used */
uint64_t ug_hpoly_vectors_bytes(uint32_t domain_size, int group);
/* The same block in two steps, for a prover sharded over GPUs: ug_hpoly_chain computes the coset evaluations of
 * ONE of the three polynomials (which = 0: A.w, 1: B.w, 2: (A.w) o (B.w)) -- ranks take different polynomials and
 * exchange slices -- and ug_hpoly_combine turns matching slices of the three vectors into h[first, first+count).
 * The evaluation vectors are in the library's device form and only meaningful to this library. ug_hpoly_combine needs
 * no coefficient matrix: hp may be NULL (then the work runs on h_out's context). */
int  ug_hpoly_chain(ug_hpoly* hp, const ug_dvec* witness, int which, ug_dvec* out_evals);
int  ug_hpoly_combine(ug_hpoly* hp, const ug_dvec* a, const ug_dvec* b, const ug_dvec* c, uint64_t first, uint64_t count,
                      ug_dvec* h_out);
/* optional: also return the three coset evaluation vectors (reference Montgomery form), for tests */
int  ug_hpoly_debug_abc(ug_hpoly* hp, void* host_a, void* host_b, void* host_c);
void ug_hpoly_destroy(ug_hpoly* hp);

/* WITNESS CHECK AGAINST THE CIRCUIT'S .r1cs (r1cs.hip; no reference counterpart: the reference proves whatever witness it is
 * given, and the host tool for the question, `snarkjs wtns check`, takes minutes at the sizes this prover is used for).
 * A zkey's section 4 holds the A and B matrices only -- the prover sets c = a o b itself --, so the C matrix comes from the .r1cs.
 *
 * THE FILE LAYOUT read here. No .r1cs from a real compiler was at hand when this was written: the layout is pinned by this
 * restatement only, and the parser (host_util.cpp) and the test writer (ultragroth_amd/synth.py: r1cs_file) are both written from it.
 * The iden3 binfile container (magic[4] | u32 version | u32 nSections | { u32 id, u64 size, bytes }*) with magic "r1cs", version 1:
 *   section 1 (header)       u32 n8 (must be 32) | prime[n8] little-endian (must be the BN254 scalar modulus r) | u32 nWires |
 *                            u32 nPubOut | u32 nPubIn | u32 nPrvIn | u64 nLabels | u32 nConstraints
 *   section 2 (constraints)  nConstraints records, each three linear combinations A, B, C; a linear combination is u32 nTerms and
 *                            nTerms x (u32 wire | coef[n8]); coef is a PLAIN little-endian integer (not Montgomery). The constraint
 *                            holds when (A.w)(B.w) = C.w mod r. nTerms = 0 is the value 0; a wire may repeat inside a combination
 *                            (the terms add).
 *   section 3 (wire -> label, nWires x u64) is not read; any other section id (custom gates) is ignored; sections are found by id,
 *   their order in the file does not matter.
 * A call fails, the message prefixed "r1cs: ", for: a missing or short section 1 or 2; n8 != 32; another prime ("not over the BN254
 * scalar field"); wire >= nWires ("constraint <k>: wire <id> out of range"); a coefficient >= r ("constraint <k>: coefficient not
 * below the field modulus"); a record that runs past the section; trailing bytes in section 2; nWires == 0; more than 2^32 - 1 terms
 * in one matrix (the offsets are u32, as in the zkey's coefficient matrix).
 *
 * ug_r1cs: the three matrices resident in HBM as CSR triples. The check runs one lane per constraint; the witness is plain 32-byte
 * integers, ANY value below 2^256, taken mod r by the products exactly as the prover takes it (the H block's rule); both sides of
 * the comparison are fully reduced first. report: failed = constraints that do not hold, first = the lowest of them, a / b / c = the
 * values A.w, B.w, C.w of constraint `first` (plain little-endian, mod r; filled only when failed > 0), device_ms = the check
 * kernel's time (ug_r1cs_check only).
 * ug_r1cs_match_hpoly answers whether the .r1cs is the circuit a zkey was made for, by probing both with one vector z of nWires
 * random field elements: A_zkey.z = A_r1cs.z and B_zkey.z = B_r1cs.z on every row below nConstraints; rows nConstraints + s,
 * 0 <= s <= n_public, of the zkey's A evaluate to z[s] (snarkjs' public rows); every other row of the zkey's A and B is empty.
 * *matrix = -1: they match; else the lowest differing row and, on that row, the first differing matrix (0 = A, 1 = B). Two
 * different rows agree on a random z with probability about 1/r. C IS NOT IN A ZKEY: an .r1cs with a wrong C matches all the same.
 * Sizes that cannot belong together (nWires != the zkey's nVars, nConstraints + n_public + 1 > domain) fail the call with
 * "r1cs: not this circuit: ...". */
typedef struct ug_r1cs ug_r1cs;
typedef struct { uint32_t n_wires, n_pub_out, n_pub_in, n_prv_in, n_constraints; uint64_t n_labels, terms[3]; } ug_r1cs_info;
typedef struct { uint64_t failed, first; uint8_t a[32], b[32], c[32]; double device_ms; } ug_r1cs_report;
int  ug_r1cs_parse_info(const void* r1cs, uint64_t size, ug_r1cs_info* out);       /* host only, no device */
/* parses (every rule above, before the first device byte), uploads through the context's staging and converts the coefficients;
 * a failed create leaves no device memory behind */
int  ug_r1cs_create(ug_ctx* ctx, const void* r1cs, uint64_t size, ug_r1cs** out);
int  ug_r1cs_get_info(const ug_r1cs* r, ug_r1cs_info* out);
/* witness[first, first + n_wires) (a shorter vector: UG_ERROR); mask: n_constraints host bytes (0 holds, 1 fails) or NULL.
 * One launch, one host wait (a failing witness: one more one-lane launch for a, b, c). */
int  ug_r1cs_check(ug_r1cs* r, const ug_dvec* witness, uint64_t first, ug_r1cs_report* out, uint8_t* mask);
/* queue only, no host wait: the result words stay on their way until ug_r1cs_check_collect, which waits for this slot's check
 * alone; may be queued on `via`'s stream (NULL: the object's context). The witness must stay as it is until the collect.
 * Slots 0 .. UG_BATCH_MAX - 1; never on a stream that is being recorded (ug_graph_begin). */
int  ug_r1cs_check_enqueue(ug_r1cs* r, const ug_dvec* witness, uint64_t first, int slot, ug_ctx* via);
int  ug_r1cs_check_collect(ug_r1cs* r, int slot, ug_r1cs_report* out);
/* The same for the `count` witnesses of a batched pass in ONE launch (r1cs_check_vectors_kernel: a lane takes one constraint for a
 * group of two witnesses, so the three matrices are walked once per group, not once per witness). Witness v is at elements
 * first + v * stride of `witness` (a shorter vector: UG_ERROR), its result goes to slot slot0 + v; 1 <= count, slot0 + count <=
 * UG_BATCH_MAX. Every slot is collected with ug_r1cs_check_collect as before, and every report is the one ug_r1cs_check gives for
 * that witness alone, bit for bit. */
int  ug_r1cs_check_vectors_enqueue(ug_r1cs* r, const ug_dvec* witness, uint64_t first, uint64_t stride, int count, int slot0, ug_ctx* via);
/* blocking, for tests and tools: reports[count]; masks: count * n_constraints host bytes (witness v's at v * n_constraints) or NULL;
 * device_ms of every report is the one launch's time. Uses slots 0 .. count - 1, which must be free. */
int  ug_r1cs_check_vectors(ug_r1cs* r, const ug_dvec* witness, uint64_t first, uint64_t stride, int count, ug_r1cs_report* reports,
                           uint8_t* masks);
int  ug_r1cs_match_hpoly(ug_r1cs* r, const ug_hpoly* hp, uint32_t n_public, int* matrix, uint64_t* row);
void ug_r1cs_destroy(ug_r1cs* r);

/* DEVELOPMENT SETUP: .r1cs + a KNOWN trapdoor -> a proving key and its verification key (setup.hip, setup_host.cpp; no reference
 * counterpart: the reference starts from a .zkey somebody else made). THE KEY IS A TEST KEY: whoever knows tau, alpha, beta,
 * gamma and the deltas forges proofs for it. It is for benchmarks, integration tests and CI, where a key must be structurally
 * real for a circuit today; it is never a substitute for a ceremony.
 *
 * The protocol is that of tests/golden/make_trapdoor_fixtures.py, which is the specification. Domain N = 2^log_domain (0: the
 * smallest that holds nConstraints + nPublic + 1 rows; at most 2^27); rows nConstraints + s, 0 <= s <= nPublic = nPubOut + nPubIn,
 * are snarkjs' public rows (A = {s: 1}). With L_k the Lagrange basis of the domain of omega = 5^((r-1)/N), per wire s:
 * u_s = sum_k A[k,s] L_k(tau), v_s, w_s likewise from B and C, K_s = beta u_s + alpha v_s + w_s;
 *   A_s = u_s G1, B1_s = v_s G1, B2_s = v_s G2, IC_s = K_s / gamma G1 (s <= nPublic),
 *   protocol 1:    C_s = K_s / delta_final G1 (s > nPublic);
 *   protocol 1337: C1 = K_s / delta_round G1 over round_signals, C2 = K_s / delta_final G1 over final_signals -- the two lists
 *                  must partition nPublic + 1 .. nVars - 1 --, rand_indx a public signal;
 *   H_k = L_k(tau / g) (tau^N - 1) / (-2 delta_final) G1, g = omega_2N.
 * A scalar of 0 gives the all-zero record. Section 4: one record per (matrix, row, wire), row first, A before B, wire ascending,
 * value coef * 2^512 mod r; repeated wires of a combination are added, a sum of 0 is left out; the public rows are included.
 * The verification key is JSON with the fields of snarkjs (protocol 1337: nPublic without the rand signal, IC without it, IC_rand).
 *
 * A call fails, the message prefixed "setup: " (or "r1cs: ", from the loader), for: tau^(2N) = 1 (tau or tau / g lies in the
 * domain); alpha, beta, gamma or a delta that is 0 mod r; a value not below r; a log_domain too small or above 27; lists that do
 * not partition the private signals; sizes that cannot be represented. Errors come back in error_msg, as in include/prover.h.
 *
 * device >= 0: Lagrange evaluation, the transposed sparse products and the fixed-base multiplications run as kernels on that
 * device; device = -1: the same steps on host threads (the comparator, and what a program without a GPU has). Both give the
 * same bytes. The six trapdoor values are plain 32-byte little-endian integers. */
typedef struct {
    uint32_t size;                      /* sizeof(ug_setup_options) */
    uint32_t protocol;                  /* 1 Groth16, 1337 UltraGroth */
    uint32_t log_domain;                /* 0: the smallest domain that fits */
    uint32_t rand_indx;                 /* protocol 1337 only */
    uint8_t  tau[32], alpha[32], beta[32], gamma[32], delta_round[32], delta_final[32];     /* protocol 1 reads delta_final only */
    const uint32_t* round_signals; uint64_t n_round;        /* protocol 1337 only */
    const uint32_t* final_signals; uint64_t n_final;
} ug_setup_options;
#define UG_SETUP_PHASES 6   /* parse + index (+ upload) | Lagrange | transposed products | G1 mult. | G2 mult. | download + assembly */
/* fills the six trapdoor values from OS entropy: uniform below r, never 0 */
int  ug_setup_draw_trapdoor(ug_setup_options* opt, char* error_msg, unsigned long long error_msg_maxsize);
/* host only: the exact size of the zkey the run writes, and an upper bound of the verification key's JSON with its final 0 */
int  ug_setup_size(const ug_setup_options* opt, const void* r1cs, uint64_t r1cs_size, uint64_t* zkey_bytes, uint64_t* vkey_bytes_max,
                   char* error_msg, unsigned long long error_msg_maxsize);
/* fills zkey (zkey_capacity >= the size query's answer) and vkey_json (0-terminated; *vkey_bytes = its length without the 0);
 * phase_ms: UG_SETUP_PHASES doubles, milliseconds per phase (device phases by stream events), or NULL */
int  ug_setup_run(const ug_setup_options* opt, const void* r1cs, uint64_t r1cs_size, int device, void* zkey, uint64_t zkey_capacity,
                  uint64_t* zkey_bytes, char* vkey_json, uint64_t vkey_capacity, uint64_t* vkey_bytes, double* phase_ms, char* error_msg,
                  unsigned long long error_msg_maxsize);
/* Test tooling, in the spirit of ug_fr_ntt / ug_field_op. ug_generator_mul: out[i] = scalars[i] * G as zkey-format affine records
 * (64 bytes for G1, 128 for G2), scalars plain 32-byte integers below r, host buffers; window: the width of the signed-digit
 * window tables, 4 .. 16, 0 = the default; kernel_ms (may be NULL): two doubles, the milliseconds of the table build and of the
 * multiplication kernels (host threads: 0 and the whole call).
 * ug_lagrange_at: out[k] = L_k(x) (coset != 0: L_k(x / omega_2N)) of the size-2^log_n domain, N plain 32-byte integers. */
int  ug_generator_mul(int device, int g2, const void* scalars, uint64_t n, int window, void* out, double* kernel_ms, char* error_msg,
                      unsigned long long error_msg_maxsize);
int  ug_lagrange_at(int device, int log_n, const void* x, int coset, void* out, char* error_msg, unsigned long long error_msg_maxsize);

/* PHASE-2 SETUP FROM A PREPARED POWERS-OF-TAU FILE: .r1cs + .ptau -> a Groth16 (protocol 1) proving key and its verification key
 * (setup_ptau.cpp, setup_points.hip; what `snarkjs zkey new` does, then optionally ONE delta contribution). No trapdoor is known
 * to this code: tau, alpha and beta stay inside the points of the ceremony.
 * OUT OF SCOPE here: UltraGroth keys (protocol 1337), which ug_ultra_setup_ptau_run below makes; in both: contribution transcripts (the zkey's section 10 is written empty, so
 * `snarkjs zkey verify` does not accept a key made here); beacons; verifying the .ptau's own ceremony. A key made without a
 * contribution has delta = 1: ANYONE forges proofs for it. A key made with a drawn delta is a single-party phase 2: it is sound
 * only if that run's delta is gone and the .ptau is honest.
 *
 * The .ptau layout, AS REMEMBERED of snarkjs' format. NO FILE OF A REAL CEREMONY HAS BEEN READ YET: this restatement is the only
 * pin, as it was for .r1cs; the reader (host_util.cpp) and the test writer (ultragroth_amd/synth.py: ptau_file) are written from it.
 * The iden3 binfile container with magic "ptau", version 1; sections are found by id, their order does not matter:
 *   section 1 (header)        u32 n8 (must be 32) | prime[n8] little-endian (must be the BN254 BASE modulus q) | u32 power |
 *                             u32 ceremonyPower
 *   section 2  tauG1          2^(power+1) - 1 G1 points     section 3  tauG2       2^power G2 points
 *   section 4  alphaTauG1     2^power G1 points             section 5  betaTauG1   2^power G1 points
 *   section 6  betaG2         1 G2 point                    section 7  contributions: not read
 *   A point is the zkey's own affine record: 64 bytes (G1) or 128 bytes (G2), coordinates little-endian in Montgomery form
 *   (R = 2^256); all-zero is infinity.
 *   sections 12, 13, 14, 15   the Lagrange forms of sections 2, 3, 4, 5, present only after `powersoftau prepare phase2`:
 *                             levels p = 0 .. power concatenated, level p = the 2^p points [L_k^(2^p)(tau)] X, so level p starts
 *                             at record 2^p - 1. Section 12 alone has one more level, p = power + 1, made from the 2^(power+1) - 1
 *                             powers the ceremony has with infinity in place of the missing top power: its point j is
 *                             [L_j(tau) - c_j tau^(2^(power+1) - 1)] G1, c_j the leading coefficient of L_j.
 * Read, for a circuit of domain N = 2^n (n chosen as ug_setup_run chooses it, or log_domain; n <= power): level n of sections
 * 12 - 15, the odd records of level n + 1 of section 12, record 0 of sections 4 and 5, section 6. Nothing else is touched and
 * nothing is copied whole: the call takes a (mapped) buffer.
 * A call fails, the message prefixed "ptau: ", for: a missing or short section 1; n8 != 32; another prime; sections 12 - 15 absent
 * ("not prepared for phase 2"); "power <p> is below the circuit's <n>"; a section shorter than the slices need; sizes that cannot
 * be represented (a power above 28). Every such rule fires before the first device byte. The slices then go through the point
 * check (ug_points_check: validate = 1 field range and curve, the default of the tools; 2 the G2 subgroup as well; 0 none):
 * "ptau: section <id> point <index>: <reason>", index counted in the section.
 *
 * The key. T, T2, aT, bT = the level-n slices of sections 12, 13, 14, 15; rows as in ug_setup_run (row nConstraints + s carries
 * A = {s: 1}); per wire s:
 *   A_s = sum_{A terms (k,s)} coef T[k]     B1_s = sum_{B terms} coef T[k]     B2_s = sum_{B terms} coef T2[k]
 *   K_s = sum_{A terms} coef bT[k] + sum_{B terms} coef aT[k] + sum_{C terms} coef T[k]
 *   IC_s = K_s (s <= nPublic), C_s = (1/delta) K_s (s > nPublic), H_k = (1/delta) (record 2k+1 of section 12, level n + 1)
 *   alpha1 = section 4 [0], beta1 = section 5 [0], beta2 = section 6, gamma2 = G2, delta1 = delta G1, delta2 = delta G2
 * delta = 1 without a contribution (what `zkey new` writes). A wire on no side and a sum that is the neutral element give the
 * all-zero record. Section 4, the headers, the section order and the JSON are ug_setup_run's. For a .ptau made from a known
 * (tau, alpha, beta) the key equals, byte for byte, ug_setup_run's for the trapdoor (tau, alpha, beta, gamma = 1, delta).
 * device >= 0: the per-wire point combinations and the delta step run as kernels; device = -1: host threads, the same bytes. */
typedef struct {
    uint32_t size;                      /* sizeof(ug_setup_ptau_options) */
    uint32_t log_domain;                /* 0: the smallest domain that fits */
    uint32_t validate;                  /* 0 no point check, 1 field range + curve, 2 the G2 subgroup as well */
    uint32_t contribute;                /* 0: delta = 1; 1: delta[] is applied; 2: a delta is drawn from OS entropy, applied, wiped and
                                           never returned or logged */
    uint8_t  delta[32];                 /* contribute = 1: plain little-endian, below r, not 0 */
} ug_setup_ptau_options;
#define UG_SETUP_PTAU_PHASES 6   /* parse + index | point check | G1 combinations | G2 combination | delta step | assembly */
typedef struct { uint32_t power, ceremony_power, prepared, max_log_domain; } ug_ptau_info;
/* host only: the header; prepared = sections 12 - 15 are there; max_log_domain = the largest domain the file serves (0: none) */
int  ug_ptau_parse_info(const void* ptau, uint64_t ptau_size, ug_ptau_info* out, char* error_msg, unsigned long long error_msg_maxsize);
/* host only: every rule of both files, the exact size of the zkey and an upper bound of the JSON with its final 0 */
int  ug_setup_ptau_size(const ug_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                        uint64_t* zkey_bytes, uint64_t* vkey_bytes_max, char* error_msg, unsigned long long error_msg_maxsize);
/* phase_ms: UG_SETUP_PTAU_PHASES doubles or NULL */
int  ug_setup_ptau_run(const ug_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                       int device, void* zkey, uint64_t zkey_capacity, uint64_t* zkey_bytes, char* vkey_json, uint64_t vkey_capacity,
                       uint64_t* vkey_bytes, double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize);
/* Test tooling for the two heavy steps, host buffers, device >= 0 or -1 (host threads); messages prefixed "setup: ".
 * ug_points_combine: out[c] = sum over the terms [col_ptr[c], col_ptr[c + 1]) of coefs[t] * points[index[t]], one zkey-format
 * record per column (64 bytes for G1, 128 for G2); col_ptr: n_cols + 1 offsets from 0, ascending; coefs plain 32-byte integers
 * below r; points: n_points zkey-format records (not validated here: ug_points_check does that). kernel_ms (may be NULL): two
 * doubles, the per-term products and the per-column sums.
 * ug_points_scale: out[i] = scalar * points[i] over n G1 records; kernel_ms (may be NULL): one double. */
int  ug_points_combine(int device, int g2, const uint32_t* col_ptr, uint64_t n_cols, const uint32_t* index, const void* coefs,
                       const void* points, uint64_t n_points, void* out, double* kernel_ms, char* error_msg,
                       unsigned long long error_msg_maxsize);
int  ug_points_scale(int device, const void* scalar, const void* points, uint64_t n, void* out, double* kernel_ms, char* error_msg,
                     unsigned long long error_msg_maxsize);

/* PHASE-2 SETUP OF AN ULTRAGROTH KEY FROM A PREPARED POWERS-OF-TAU FILE: .r1cs + .ptau + the commitment rounds -> a protocol-1337
 * proving key and its verification key (setup_ptau.cpp, setup_points.hip), optionally with ONE contribution to each of the two
 * deltas. ug_setup_ptau_run beside it stays what it is; everything it says about the .ptau, its layout ("AS REMEMBERED"), its
 * rules and messages, the point check and what is OUT OF SCOPE (transcripts, beacons, the .ptau's own ceremony) holds here.
 * contribute = 0 leaves BOTH deltas 1: ANYONE forges proofs for such a key. contribute = 2 is a single-party phase 2 with no
 * transcript: the key is sound only if that run's two deltas are gone and the .ptau is honest.
 *
 * Which signal is committed in which round is what UltraGroth's soundness rests on, and this call takes it from the caller:
 * rand_indx, a public signal (1 .. nPublic), carries the challenge; round_signals are committed before it, final_signals after;
 * the two lists must partition the private signals nPublic + 1 .. nVars - 1 (an empty list is legal). The rules and their
 * messages are ug_setup_run's for protocol 1337. A delta must be below r and not 0 ("setup: delta_round is 0 mod r", "setup:
 * delta_final is not below the field modulus"). Every rule of the options and of both files fires before the first device byte.
 *
 * The key, in ug_setup_ptau_run's notation (T, T2, aT, bT, K_s; P = level n + 1 of section 12):
 *   sections 5, 6, 7   A, B1, B2 as for Groth16
 *   section 3          IC_s = K_s for every s <= nPublic, the rand signal included
 *   section 8          C1[i] = (1 / delta_round) K_(round_signals[i])      section 10   round_signals, in the order given
 *   section 9          C2[i] = (1 / delta_final) K_(final_signals[i])      section 11   final_signals, in the order given
 *   section 12         H_k = (1 / delta_final) P[2k + 1]                   section 13   contributions: empty
 *   header             alpha1, beta1, beta2 from the .ptau; gamma2 = G2; delta_c1 = delta_round (G1, G2); delta_c2 = delta_final (G1, G2)
 * The container, the section order and the JSON (nPublic without the rand signal, IC without it, IC_rand, vk_delta_c1_2,
 * vk_delta_c2_2) are ug_setup_run's for protocol 1337. For a .ptau made from a known (tau, alpha, beta) the key and the JSON
 * equal, byte for byte, ug_setup_run's for protocol 1337 and the trapdoor (tau, alpha, beta, gamma = 1, delta_round, delta_final).
 * device >= 0: the point combinations run as ug_setup_ptau_run's kernels and the whole delta step -- C1, C2 and H, gathered
 * through the two lists -- is ONE launch (scale_segments_kernel); device = -1: host threads, the same bytes. */
typedef struct {
    uint32_t size;                      /* sizeof(ug_ultra_setup_ptau_options) */
    uint32_t log_domain;                /* 0: the smallest domain that fits */
    uint32_t validate;                  /* 0 no point check, 1 field range + curve, 2 the G2 subgroup as well */
    uint32_t contribute;                /* 0: both deltas 1; 1: delta_round[] and delta_final[] are applied; 2: both are drawn
                                           independently from OS entropy, applied, wiped and never returned or logged */
    uint8_t  delta_round[32], delta_final[32];              /* contribute = 1: plain little-endian, below r, not 0 */
    uint32_t rand_indx;
    uint32_t reserved;                  /* 0 */
    const uint32_t* round_signals; uint64_t n_round;
    const uint32_t* final_signals; uint64_t n_final;
} ug_ultra_setup_ptau_options;
/* host only: every rule of the options and of both files, the exact size of the zkey and an upper bound of the JSON with its final 0 */
int  ug_ultra_setup_ptau_size(const ug_ultra_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                              uint64_t ptau_size, uint64_t* zkey_bytes, uint64_t* vkey_bytes_max, char* error_msg,
                              unsigned long long error_msg_maxsize);
/* phase_ms: UG_SETUP_PTAU_PHASES doubles (the phases of ug_setup_ptau_run) or NULL */
int  ug_ultra_setup_ptau_run(const ug_ultra_setup_ptau_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                             uint64_t ptau_size, int device, void* zkey, uint64_t zkey_capacity, uint64_t* zkey_bytes, char* vkey_json,
                             uint64_t vkey_capacity, uint64_t* vkey_bytes, double* phase_ms, char* error_msg,
                             unsigned long long error_msg_maxsize);
/* Test tooling for the delta step of an UltraGroth key, host buffers, device >= 0 or -1 (host threads); messages prefixed "setup: ".
 * n_segments <= 3 segments over ONE array of n_points G1 records: segment s writes count records, scalar * points[index[i]], or
 * scalar * points[i] when index is NULL (count <= n_points then); every index must be below n_points. out: the segments' records
 * one segment after the other. A scalar (plain, below r) of 1 copies the gathered records, 0 gives all-zero records; infinity in
 * gives infinity out. On the device all segments are one launch; kernel_ms (may be NULL): one double. */
typedef struct {
    const void* scalar;
    const uint32_t* index;              /* count indexes into points, or NULL */
    uint64_t count;
} ug_scale_segment;
int  ug_points_scale_segments(int device, int n_segments, const ug_scale_segment* segments, const void* points, uint64_t n_points,
                              void* out, double* kernel_ms, char* error_msg, unsigned long long error_msg_maxsize);

/* CHECKING A KEY AGAINST ITS CIRCUIT AND POWERS OF TAU (zkey_verify.cpp, zkey_verify.hip; what `snarkjs zkey verify` answers about
 * the key's POINTS; no reference counterpart: the reference starts from a .zkey somebody else made). Given a circuit's .r1cs, a
 * .ptau prepared for phase 2 and a Groth16 (protocol 1) .zkey, the call says whether sections 2 - 9 of the key are the ones
 * ug_setup_ptau_run gives for these files under ONE delta, which is not known to this code: the key is then A phase-2 descendant
 * of `zkey new` for SOME delta. OUT OF SCOPE: who contributed -- section 10's transcript, beacons, the .ptau's own ceremony
 * (ug_ptau_prepare_run's check mode covers sections 12 - 15 against 2 - 5) -- and UltraGroth keys, which are refused with
 * "zkey: protocol 1337 keys are not checked".
 *
 * The relations (notation of ug_setup_ptau_run, P = level n + 1 of section 12). rho: one weight below 2^128
 * per wire, sigma: one per row of the domain, drawn from getrandom in every call and never derived from the inputs; rho^pub = rho on
 * wires 0 .. nPublic, rho^priv the rest; a^m = A rho^m, b^m = B rho^m, c^m = C rho^m over the rows (the public rows in a^pub);
 * K^m = MSM(a^m, bT) + MSM(b^m, aT) + MSM(c^m, T); a = a^pub + a^priv, b likewise. In this order:
 *   0  section 2   alpha1, beta1, beta2 are the .ptau's section 4 [0], 5 [0], 6 by bytes; delta1, delta2, gamma2 are not infinity;
 *                  e(delta1, G2) = e(G1, delta2)                          "zkey: header: <field> ..."
 *   1  section 4   byte for byte the section ug_setup_run writes for the .r1cs     "zkey: section 4 record <i>: does not match the circuit"
 *   2  section 5   MSM(rho, A) = MSM(a, T)                    3  section 6   MSM(rho, B1) = MSM(b, T)
 *   4  section 7   MSM(rho, B2) = MSM(b, T2)                  5  section 3   e(MSM(rho^pub, IC), gamma2) = e(K^pub, G2)
 *   6  section 8   e(MSM(rho^priv, C), delta2) = e(K^priv, G2)
 *   7  section 9   e(MSM(sigma, H), delta2) = e(MSM(sigma, odd records of P), G2)
 * with "zkey: section <id>: does not match the circuit and the powers of tau" for sections 3, 5, 6, 7 and the same plus " under the
 * key's delta" for 8 and 9. gamma2 is the key's own (snarkjs writes G2; ug_setup_run's keys have any gamma). All relations are
 * evaluated even after one fails; error_msg holds the message of the first that fails in the order above, first_failed its section.
 * A deviating section is accepted with probability at most 2^-128 per relation, GIVEN that every point lies in its group of order r:
 * so every point of the key and of the slices goes through the point check first (ug_points_check; host threads for device = -1),
 * the G2 points at level `validate`. validate = 2 (the tool's default) checks the G2 subgroup; validate = 1 is for timing and its
 * report says subgroup_checked = 0: an answer of UG_OK is then NOT "valid".
 *
 * Returns UG_OK: valid; UG_ZKEY_INVALID: failed_sections has bit <id> set for every failing section 2 - 9; UG_ERROR: refused --
 * a file that cannot be read, sizes that do not belong together (the loaders' texts under "r1cs: " / "ptau: " / "zkey: "; "zkey:
 * header: nVars ..." and the like), or a bad point, with ug_zkey_check's message for the key ("zkey: section <id> point <i>:
 * <reason>", "zkey: header point <name>: <reason>") and ug_setup_ptau_run's for the .ptau. Every size and header rule fires before
 * the first device byte. device >= 0: the fold and the MSMs run on the device, one section's bases resident at a time;
 * device = -1: the same relations on host threads (the comparator, and what a machine without a GPU has). The pairings run on
 * host threads either way. The files are only read: the call takes (mapped) buffers. */
#define UG_ZKEY_INVALID 2
typedef struct {
    uint32_t size;                      /* sizeof(ug_zkey_verify_options) */
    uint32_t validate;                  /* 2: field range, curve and G2 subgroup of every point; 1: without the subgroup (timing only) */
} ug_zkey_verify_options;
typedef struct {
    uint32_t failed_sections;           /* bit <id> for every section 2 - 9 that fails */
    int32_t  first_failed;              /* the section of the first failing relation in the order above, 0: none */
    uint32_t subgroup_checked;          /* 1: the G2 points passed the subgroup rule (validate = 2) */
    uint32_t reserved;
    uint64_t peak_device_bytes;         /* device memory in use at its peak, above what was in use when the call began (device >= 0) */
    double   fold_kernel_ms;            /* the fold kernel alone (host threads: the fold's wall time) */
} ug_zkey_verify_report;
#define UG_ZKEY_VERIFY_PHASES 8  /* parse + header + section 4 | point check | weights | fold | slice products | key products | H products | pairings */
int  ug_zkey_verify_run(const ug_zkey_verify_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                        const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out, double* phase_ms, char* error_msg,
                        unsigned long long error_msg_maxsize);
/* Test tooling for the fold, host buffers, device >= 0 or -1 (host threads); messages prefixed "r1cs: ". rho: nWires plain 32-byte
 * integers, ANY value below 2^256, taken mod r as a witness is; log_domain 0: the smallest domain that fits. out: SIX vectors of
 * N = 2^log_domain plain canonical integers, a^pub, b^pub, c^pub, a^priv, b^priv, c^priv: row k < nConstraints holds the sums of
 * its A, B, C terms times rho over the wires 0 .. nPublic and over the others; row nConstraints + s, s <= nPublic, holds rho_s mod r
 * in a^pub and 0 elsewhere; the rows above hold 0. kernel_ms (may be NULL): the kernel's time. */
int  ug_r1cs_fold(const void* r1cs, uint64_t r1cs_size, const void* rho, uint32_t log_domain, int device, void* out, double* kernel_ms,
                  char* error_msg, unsigned long long error_msg_maxsize);
/* CHECKING AN ULTRAGROTH KEY (protocol 1337) against its circuit and powers of tau: ug_zkey_verify_run's question for the keys
 * ug_ultra_setup_ptau_run makes, beside it (a Groth16 key is refused here with "zkey: zkey file is not ultragroth", as an UltraGroth
 * key is refused there). Valid: sections 2 - 12 are the ones ug_ultra_setup_ptau_run gives for these files under ONE delta_round and
 * ONE delta_final, neither known to this code. OUT OF SCOPE: transcripts, beacons, the .ptau's own ceremony, and -- when no spec is
 * given -- WHO CHOSE THE ROUNDS: the key's own lists are then taken as they are, and which signal is committed before the challenge
 * is what the protocol's soundness rests on.
 * rho, sigma as in ug_zkey_verify_run. The wires fall in three classes: pub = 0 .. nPublic, round = the key's section 10, final = its
 * section 11; a^m, b^m, c^m, K^m as there for m in {pub, round, final}; a = a^pub + a^round + a^final. In this order, all evaluated:
 *   0  section 2    alpha1, beta1, beta2 are the .ptau's by bytes; gamma2, delta_c1, delta_c2 (G1 and G2 parts) are not infinity;
 *                   e(delta_c1_1, G2) = e(G1, delta_c1_2) and the same for delta_c2            "zkey: header: ..."
 *   1  section 4    byte for byte, as for Groth16
 *   2  10, 11       with a spec (check_spec = 1): rand_indx and each list equal the spec's     "zkey: header: rand_indx does not match the
 *                   spec", "zkey: section 10: does not match the spec" (likewise 11)
 *   3 - 5  5, 6, 7  as for Groth16                      6  section 3   e(MSM(rho^pub, IC), gamma2) = e(K^pub, G2)
 *   7  section 8    e(MSM(rho[round_signals[i]], C1[i]), delta_c1_2) = e(K^round, G2)           "... under the key's round delta"
 *   8  section 9    the same over the final list with delta_c2_2                                "... under the key's final delta"
 *   9  section 12   e(MSM(sigma, H), delta_c2_2) = e(MSM(sigma, odd records of P), G2)          "... under the key's final delta"
 * An empty list: its relation holds trivially and K^m must be infinity. REFUSED (UG_ERROR), before the first device byte: every
 * refusal of ug_zkey_verify_run; a rand_indx that is not public, lists that do not partition the private signals (ug_setup_run's
 * texts under "zkey: "; n_indexes_c1 + n_indexes_c2 = nVars - nPublic - 1 is part of that rule). Every point of the key and of
 * the slices goes through the point check first ("zkey: header point delta_c1_2: ..."); validate = 1 reports subgroup_checked = 0
 * and is not "valid". failed_sections has bit <id> set for the sections 2 - 12. device >= 0: the fold (r1cs_fold_classes_kernel) and
 * the MSMs run on the device, one section's bases resident at a time; the weights of a list's signals are gathered on the host (32
 * bytes per private signal); device = -1: host threads. Pairings run on host threads either way. phase_ms: UG_ZKEY_VERIFY_PHASES. */
typedef struct {
    uint32_t size;                      /* sizeof(ug_ultra_zkey_verify_options) */
    uint32_t validate;                  /* 2 | 1 as ug_zkey_verify_options.validate */
    uint32_t check_spec;                /* 1: the key's rand_indx and lists must equal the ones below; 0: they are not read */
    uint32_t rand_indx;
    const uint32_t* round_signals; uint64_t n_round;
    const uint32_t* final_signals; uint64_t n_final;
} ug_ultra_zkey_verify_options;
int  ug_ultra_zkey_verify_run(const ug_ultra_zkey_verify_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                              uint64_t ptau_size, const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out,
                              double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize);
/* Test tooling for the fold with a class per wire; as ug_r1cs_fold, but cls: nWires bytes, each 0, 1 or 2 (any map: the public
 * wires need not be class 0 here), and out: ELEVEN vectors of N integers: vector 3 m + t is the sum of matrix t (A, B, C) over the
 * wires of class m; vector 9 is a, 10 is b (the sums over all wires). The public rows hold rho_s in vectors 0 and 9.
 * ug_r1cs_fold_classes_dvec: the device form; cls: the class bytes packed 32 to an element; out: 11 * 2^log_domain elements. */
int  ug_r1cs_fold_classes(const void* r1cs, uint64_t r1cs_size, const void* rho, const void* cls, uint32_t log_domain, int device, void* out,
                          double* kernel_ms, char* error_msg, unsigned long long error_msg_maxsize);
int  ug_r1cs_fold_classes_dvec(ug_r1cs* r, const ug_dvec* rho, const ug_dvec* cls, uint32_t n_public, uint32_t log_domain, ug_dvec* out,
                               double* kernel_ms);
/* The device forms the check is made of. ug_r1cs_fold_dvec: the fold of a resident circuit over a resident rho into `out`, EIGHT
 * vectors of 2^log_domain elements: the six above, then a = a^pub + a^priv and b, each an MSM scalar vector where it lies
 * (ug_schedule_build over its range); one launch, one host wait. ug_bases_create_every_g1: the G1 set of the records first,
 * first + step, ... of n_records host records (H's sources are the odd records of a level: first 1, step 2), gathered on the device. */
int  ug_r1cs_fold_dvec(ug_r1cs* r, const ug_dvec* rho, uint32_t n_public, uint32_t log_domain, ug_dvec* out, double* kernel_ms);
int  ug_bases_create_every_g1(ug_ctx* ctx, const void* host_points, uint64_t n_records, uint64_t first, uint64_t step, uint64_t global_first,
                              ug_bases** out);

/* NAMING THE WRONG RECORDS OF A FAILING SECTION (zkey_verify_host.cpp; setup_points.hip: ratio_block_sums_kernel; pairing.hip:
 * ratio_judge_kernel). ug_zkey_verify_run answers "invalid: sections 8, 9" and nothing finer.
 * ug_zkey_locate_run / ug_ultra_zkey_locate_run sit BESIDE the two verify entries, which keep their signatures, struct sizes,
 * refusals, messages and verdicts: on the same files they give the same return code, ug_zkey_verify_report and error_msg
 * (first_failed and the first failing relation's message included), and in addition a ug_zkey_locate_report with one entry per
 * failing POINT section -- 3, 5, 6, 7, each C section and H -- in that order. Locating starts after the verdict is known: a valid key,
 * or one whose only failures are sections 2, 4, 10 or 11, costs nothing extra and reports n_sections = 0. Section 4 already names its
 * record and the header has no records: neither gets an entry. Expected records are made only for sections that failed, one
 * section at a time (made, tested, freed).
 *   sections 5, 6, 7       method UG_LOCATE_BYTES: the expected records are the combination of the circuit's columns over T and T2
 *                          (ug_points_combine's), canonical, so a byte comparison names every wrong record: exact = 1 always,
 *                          bad_records the full count, bad_blocks = resolved_blocks = the blocks that hold one.
 *   section 3, C sections  method UG_LOCATE_RATIO: record X_s against K_s = the combination over (bT, aT, T) through A, B, C, with
 *                          e(X_s, Q) = e(K_s, G2); Q = the key's gamma2 for section 3 (ug_setup_run's keys have any gamma), the
 *                          section's delta (G2 part) for a C section.
 *   H (9, or 12)           method UG_LOCATE_RATIO: H_i against the odd record 2 i + 1 of P, Q = the last delta.
 * A ratio section whose Q is the point at infinity (a header failure) gets no entry.
 * An index is the record's place IN ITS SECTION: for section 3, 5, 6, 7 the wire; for a Groth16 key's section 8 record i is wire
 * nPublic + 1 + i; for an UltraGroth key's section 8 record i is wire round_signals[i] (section 10), for its section 9 wire
 * final_signals[i] (section 11); for H the row.
 *
 * The ratio test (ug_points_ratio_mask is the test tooling for it alone, device >= 0 or -1, messages prefixed "setup: "): given n
 * pairs (X_i, Y_i) of G1 records that passed the point check (all-zero = infinity) and a G2 record Q, not infinity and in the
 * subgroup, it finds every i with e(X_i, Q) != e(Y_i, G2). Both infinity holds, exactly one is wrong. Two levels:
 *   blocks    256 consecutive records (the last may be short); one weight below 2^128 per record from getrandom, fresh in every call
 *             and never derived from the inputs; block j HOLDS when e(sum w_i X_i, Q) = e(sum w_i Y_i, G2). A block with a wrong
 *             record holds with probability at most 2^-128 (the argument of ug_zkey_verify_run's relations).
 *   records   only the first max_blocks FAILING blocks are resolved, in index order (0: the default, 64 -- 16 384 records in one
 *             launch): each of their records by its own two pairings, no weights: exact.
 * exact = 1: every failing block was resolved and bad_records is the total. exact = 0: more blocks fail than were resolved;
 * bad_records counts the resolved ones only -- when every resolved block fails in every record, the section belongs to another
 * delta or tau, not to a few bad records. device = -1 runs both levels on host threads and gives the same answers.
 * ug_points_ratio_mask: record_mask (capacity n bytes) receives one byte per record of the resolved blocks, block after block
 * (resolved_records of them; 1 = wrong), block_mask one byte per block (1 = the block fails). */
#define UG_RATIO_LISTED 16
typedef struct {
    uint64_t blocks, bad_blocks, resolved_blocks;
    uint64_t bad_records;               /* over the resolved blocks; the total when exact */
    uint64_t resolved_records;          /* bytes written to record_mask */
    uint32_t exact;
    uint32_t n_listed;                  /* the first wrong records, ascending: at most UG_RATIO_LISTED */
    uint64_t index[UG_RATIO_LISTED];
    double   kernel_ms[2];              /* ratio_block_sums_kernel; ratio_judge_kernel over both levels (host threads: wall time) */
} ug_ratio_report;
int  ug_points_ratio_mask(int device, const void* x, const void* y, uint64_t n, const void* q, uint64_t max_blocks, void* record_mask,
                          void* block_mask, ug_ratio_report* out, char* error_msg, unsigned long long error_msg_maxsize);

#define UG_LOCATE_BYTES 0
#define UG_LOCATE_RATIO 1
#define UG_ZKEY_LOCATE_SECTIONS 7       /* 3, 5, 6, 7, 8, 9 and, for an UltraGroth key, 12 */
#define UG_ZKEY_LOCATE_LISTED 1024      /* the largest max_listed */
typedef struct {
    uint32_t size;                      /* sizeof(ug_zkey_locate_options) */
    uint32_t validate;                  /* as ug_zkey_verify_options.validate */
    uint32_t max_listed;                /* wrong records listed per section; 0: 16; above UG_ZKEY_LOCATE_LISTED: refused */
    uint32_t max_blocks;                /* failing blocks resolved per ratio section; 0: 64 */
} ug_zkey_locate_options;
typedef struct {
    uint32_t size;                      /* sizeof(ug_ultra_zkey_locate_options) */
    uint32_t validate, check_spec, rand_indx;                       /* as ug_ultra_zkey_verify_options */
    const uint32_t* round_signals; uint64_t n_round;
    const uint32_t* final_signals; uint64_t n_final;
    uint32_t max_listed, max_blocks;    /* as ug_zkey_locate_options */
} ug_ultra_zkey_locate_options;
typedef struct {
    uint32_t section;                   /* the section's id */
    uint32_t method;                    /* UG_LOCATE_BYTES | UG_LOCATE_RATIO */
    uint64_t records;                   /* records of the section */
    uint64_t blocks, bad_blocks, resolved_blocks, bad_records;
    uint32_t exact;
    uint32_t n_listed;                  /* entries of index[]: the first max_listed wrong records, ascending */
    double   kernel_ms[2];              /* as ug_ratio_report (0 for UG_LOCATE_BYTES) */
    uint64_t index[UG_ZKEY_LOCATE_LISTED];
} ug_zkey_locate_section;
typedef struct {
    uint32_t n_sections;                /* entries of section[], in the order 3, 5, 6, 7, the C sections, H */
    uint32_t reserved;
    double   locate_ms;                 /* everything after the verdict (0 when nothing had to be located) */
    ug_zkey_locate_section section[UG_ZKEY_LOCATE_SECTIONS];
} ug_zkey_locate_report;
/* out, phase_ms, error_msg: exactly ug_zkey_verify_run's / ug_ultra_zkey_verify_run's. located (may not be NULL) is zeroed by a refusal. */
int  ug_zkey_locate_run(const ug_zkey_locate_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau, uint64_t ptau_size,
                        const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out, ug_zkey_locate_report* located,
                        double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize);
int  ug_ultra_zkey_locate_run(const ug_ultra_zkey_locate_options* opt, const void* r1cs, uint64_t r1cs_size, const void* ptau,
                              uint64_t ptau_size, const void* zkey, uint64_t zkey_size, int device, ug_zkey_verify_report* out,
                              ug_zkey_locate_report* located, double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize);

/* PREPARING A POWERS-OF-TAU FILE FOR PHASE 2: sections 2 - 5 -> sections 12 - 15 (ptau_prepare.cpp, ptau_prepare.hip; what
 * `snarkjs powersoftau prepare phase2` does), and the check that a file's sections 12 - 15 ARE the Lagrange forms of its sections
 * 2 - 5, which ug_setup_ptau_run takes on trust. The layout is the one restated above, AS REMEMBERED of snarkjs' format: NO FILE OF
 * A REAL CEREMONY HAS BEEN READ YET, and that caveat carries over unchanged to the sections this writes.
 * OUT OF SCOPE: contribution transcripts, beacons, verifying the ceremony's own contributions (section 7 is copied, not read).
 *
 * The transform. For a level p with N = 2^p, omega = 5^((r - 1) / N) and the points P_0 .. P_(N-1) = the first N records of a
 * section:  out[k] = (1 / N) sum_j omega^(-j k) P_j,  which is the level's point k, [L_k^(2^p)(tau)] X, when P_j = [tau^j] X.
 * Section 12's padded level power + 1 is the same transform of the 2^(power+1) - 1 records of section 2 with infinity as the last
 * input. device >= 0: a decimation-in-time radix-2 transform, one launch per stage, every butterfly a full-length product of a
 * point by a twiddle; sections 12, 14, 15 of a level share the launches. device = -1: host threads, the same bytes (affine records
 * are canonical).
 * Prepare (mode 0). The output is the input's sections other than 12 - 15, in the input's order, then 12, 13, 14, 15 in the layout
 * above; sections 12 - 15 of the input are dropped and made again. power = p' below the file's own cuts the file first: sections
 * 2 - 5 to their first 2^(p'+1) - 1, 2^p', 2^p', 2^p' records, the header's power to p' (ceremonyPower stays), every other section
 * copied; the padded level of the cut file is made from the cut section 2 with infinity in the last place, as for any file.
 * Check (mode 1). Nothing is written (out may be NULL). The call succeeds when all four sections equal the recomputed ones, and
 * fails with "ptau: section <id> point <index>: does not match the powers" for the first mismatch, in section order, index
 * counted in the section; "ptau: not prepared for phase 2" when the sections are absent. A check is of the file's own power.
 * A call fails, the message prefixed "ptau: ", for: every header rule of ug_setup_ptau_run; a section 2 - 5 (in a check also
 * 12 - 15) that is missing or shorter than its record count needs; "power <p'> is above the file's <p>"; a power of 28 (the
 * padded level would be a transform of 2^29 points, and r - 1 has only 28 factors of 2: cut such a file); an output buffer that is
 * too small -- all of these before the first device byte, and all of them by ug_ptau_prepare_size, which is host only; a level that
 * does not fit the device's free memory, "ptau: level <p> needs <bytes> on the device", before the first kernel of that level.
 * The records of sections 2 - 5 that are read go through the point check (ug_points_check) with ug_setup_ptau_run's message. */
typedef struct {
    uint32_t size;                      /* sizeof(ug_ptau_prepare_options) */
    uint32_t power;                     /* 0: the file's own; p' below the file's: the file is cut to p' first */
    uint32_t validate;                  /* 0 | 1 | 2 as ug_setup_ptau_options.validate, over the records of sections 2 - 5 that are read */
    uint32_t mode;                      /* 0 prepare: write a file; 1 check: recompute sections 12 - 15 and compare with the file's own */
} ug_ptau_prepare_options;
#define UG_PTAU_PREPARE_PHASES 5 /* parse + copied sections | point check | G1 levels (12, 14, 15) | G2 levels (13) | comparison (a check only:
                                    the comparisons run after each level, their time is taken out of the levels' phases) */
/* host only: every rule that needs no point; out_bytes: the size of the prepared file (0 for a check) */
int  ug_ptau_prepare_size(const ug_ptau_prepare_options* opt, const void* ptau, uint64_t ptau_size, uint64_t* out_bytes, char* error_msg,
                          unsigned long long error_msg_maxsize);
/* phase_ms: UG_PTAU_PREPARE_PHASES doubles or NULL; the levels' times are wall times with their uploads and downloads */
int  ug_ptau_prepare_run(const ug_ptau_prepare_options* opt, const void* ptau, uint64_t ptau_size, int device, void* out,
                         uint64_t out_capacity, uint64_t* out_bytes, double* phase_ms, char* error_msg, unsigned long long error_msg_maxsize);
/* Test tooling: ONE transform of size 2^log_n (log_n <= 28) over n_given <= 2^log_n zkey-format records, the rest infinity; out:
 * 2^log_n records (64 bytes for G1, 128 for G2). kernel_ms (may be NULL): two doubles, the 1 / N products and the stages. */
int  ug_points_intt(int device, int g2, int log_n, const void* points, uint64_t n_given, void* out, double* kernel_ms, char* error_msg,
                    unsigned long long error_msg_maxsize);

/* In-place size-2^logn transform of a host buffer of Montgomery Fr elements, natural order in and out.
 * inverse != 0 also scales by 1/n. */
int  ug_fr_ntt(ug_ctx* ctx, void* host_data, int logn, int inverse);
/* out[i] = a[i] (op) b[i] on n Montgomery elements of the chosen field (host buffers) */
int  ug_field_op(ug_ctx* ctx, int field, int op, void* out, const void* a, const void* b, uint64_t n);

/* Tooling for synthetic circuits (bench.py, tests): host_out[i] = (seed + i) * G as zkey-format affine
 * records, G given as one such record (64 bytes for G1, 128 for G2). Not part of the reference interface. */
int  ug_synth_points(ug_ctx* ctx, int g2, const void* generator_record, uint64_t seed, uint64_t n, void* host_out);

/* CAPTURED LAUNCH SEQUENCES (one hipGraph per created prover and witness buffer; no reference counterpart -- the reference's
 * prove, src/groth16.cpp:48-203, is one fixed sequence of calls, and so is this library's: no launch depends on a host read-back).
 * ug_graph_begin puts ctx's stream into capture and forks ctx2's stream (may be NULL) off it; whatever the library queues on the
 * two contexts until ug_graph_end -- schedules, products, ug_hpoly_run, ug_ctx_wait edges -- is recorded instead of run, the timing
 * events included (as event-record nodes: ug_ctx_timings / ug_ctx_kernel_stats keep working under replay). Calls that wait
 * for the device (ug_ctx_sync, _collect, blocking products, uploads) must not be made on a capturing context. ug_graph_end
 * instantiates the graph and takes the queued products out of the contexts; ug_graph_launch puts them back and launches on ctx's
 * stream: collect as after the eager calls, ctx FIRST. ug_graph_valid: 0 once any per-proof device buffer of the process has
 * been re-allocated since the capture (schedules, workspaces): the caller then drops the graph and captures again.
 * ug_graph_abort ends a capture that failed half way (nothing was queued). */
typedef struct ug_graph ug_graph;
int      ug_graph_begin(ug_ctx* ctx, ug_ctx* ctx2);
int      ug_graph_end(ug_ctx* ctx, ug_graph** out);
void     ug_graph_abort(ug_ctx* ctx);
int      ug_graph_valid(const ug_graph* g);
uint64_t ug_graph_nodes(const ug_graph* g);
int      ug_graph_launch(ug_graph* g);
void     ug_graph_destroy(ug_graph* g);

/* milliseconds of device time spent in the MSM and H-polynomial parts since the last reset
 * (the MSM | FFT split the reference prints in src/ultra_groth.cpp:199-335) */
int  ug_ctx_timings(ug_ctx* ctx, double* msm_ms, double* fft_ms, int reset);

/* HIP events (recorded on the launch stream) around the launches of the kernels the roofline is reported for:
 * which = 0 the G1 bucket accumulation, 1 the G2 bucket accumulation, 2 the NTT pass kernel. Average launch duration in
 * ms since the last reset, the launch count, and the units processed ((point, window) entries; NTT points per pass).
 * The statistics of a context are collected from its first call with reset != 0 on (an event pair around a launch costs
 * 10-25 us of idle device: a caller that never asks never pays). A captured launch sequence (ug_graph_*) holds the event pairs
 * that were on when it was captured. */
int  ug_ctx_kernel_stats(ug_ctx* ctx, int which, double* launch_ms_avg, uint64_t* launches, uint64_t* units, int reset);

#ifdef __cplusplus
}
#endif
#endif
