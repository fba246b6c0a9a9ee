/* verifier.h -- proof verification with the contract of the reference's src/verifier.h:1-46: the same two entry points,
 * argument order and result codes. Implemented as host code inside libultragroth_hip.so
 * (ultragroth_amd/csrc/verifier_api.cpp). */
#ifndef ULTRAGROTH_AMD_VERIFIER_H
#define ULTRAGROTH_AMD_VERIFIER_H

#ifdef __cplusplus
extern "C" {
#endif

/* result codes (src/verifier.h:9-11) */
enum {
    VERIFIER_VALID_PROOF = 0,      /* the pairing equation holds                           */
    VERIFIER_INVALID_PROOF = 1,    /* it does not (or a point is not on its curve)         */
    VERIFIER_ERROR = 2             /* malformed input; error_msg says which part           */
};

/* All three texts are NUL-terminated JSON in the snarkjs layout: proof.json, public.json, verification_key.json.
 * Messages on VERIFIER_ERROR: "invalid proof data", "invalid inputs data", "invalid verification key data",
 * "len(inputs)+1 != len(vk.IC)" (src/verifier.cpp:16-146, src/groth16.cpp:318-320).
 * Differences from the reference: points that are not on their curve give VERIFIER_INVALID_PROOF (the reference
 * evaluates the pairing on them regardless), and ultra_groth_verify does not print "inputs.size(): N" on stdout
 * (src/ultra_groth.cpp:591). error_msg may be NULL. */
int groth16_verify(const char *proof, const char *inputs, const char *verification_key, char *error_msg, unsigned long error_msg_maxsize);

/* UltraGroth: proof fields pi_a, pi_b, pi_f, pi_r with protocol "ultragroth"; key fields vk_delta_c1_2, vk_delta_c2_2 and
 * IC_rand; the length error reads "len(inputs) != len(vk.IC)" (src/ultra_groth.cpp:585-587). */
int ultra_groth_verify(const char *proof, const char *inputs, const char *verification_key, char *error_msg, unsigned long error_msg_maxsize);

/* ---- additions: many proofs under one key --------------------------------------------------------------------------
 * verdicts[i] is what groth16_verify / ultra_groth_verify returns for (proofs[i], inputs[i], verification_key), with one
 * exception: small-exponent batching accepts a batch that holds an invalid proof with probability at most 2^-128 (the
 * proofs are combined with 128-bit scalars drawn from the system's random source for every call, never from the inputs).
 * One Miller loop per proof and the scalar multiples run on `device` (ultragroth_amd/csrc/pairing.hip); the host adds
 * three (four) Miller loops and ONE final exponentiation per accepted pass of up to 65536 proofs. A rejected pass is
 * searched down its tree of partial products, kept from the device pass: two more checks per level and bad proof, and the
 * single-proof verifier for the at most 16 proofs of a failing node at the bottom.
 * A proof that does not parse, or whose input count is wrong, gets VERIFIER_ERROR; one with a point off its curve
 * VERIFIER_INVALID_PROOF, both without a pairing. A proof whose pi_b is on the twist but outside the subgroup of order r
 * is not batched (the pairing is not bilinear in the scalar there): the single-proof verifier decides, and it decides
 * every proof when the key itself holds such a point.
 * device < 0: the same protocol on host threads, no GPU needed.
 * Returns VERIFIER_ERROR for null arguments, count < 0, a key that does not parse (the single call's messages) or a device
 * error; verdicts is then untouched. Else VERIFIER_VALID_PROOF when every verdict is, else VERIFIER_INVALID_PROOF with
 * error_msg = "proof <first bad index>: <reason>". count == 0 is valid. stats may be NULL.
 * These two calls take their options from the environment: ULTRAGROTH_VERIFY_JUDGE=1 switches the judge (below) on with the
 * library's search_width and judge_min, unset or 0 leaves everything as described here; any other value fails the call with
 * a message that names the variable. They write the 40 bytes of ug_verify_batch_stats, whatever the setting. */
typedef struct {
    unsigned long long batch_checks;   /* final exponentiations of batch equations (1 per accepted pass)              */
    unsigned long long single_checks;  /* proofs handed to the single-proof verifier                                  */
    unsigned long long off_subgroup;   /* ... of which because pi_b is outside the subgroup                           */
    double device_ms, host_ms;         /* wall time of the device passes (uploads and downloads included); the rest   */
} ug_verify_batch_stats;
int ug_groth16_verify_batch(int device, int count, const char *const *proofs, const char *const *inputs,
                            const char *verification_key, int *verdicts, ug_verify_batch_stats *stats,
                            char *error_msg, unsigned long error_msg_maxsize);
int ug_ultra_groth_verify_batch(int device, int count, const char *const *proofs, const char *const *inputs,
                                const char *verification_key, int *verdicts, ug_verify_batch_stats *stats,
                                char *error_msg, unsigned long error_msg_maxsize);

/* ---- the judge: suspect proofs decided on the device ------------------------------------------------------------------
 * The search of a rejected pass and the single-proof verifier behind it are host work whose amount the sender of the
 * proofs decides (1 % bad proofs among 2^14: ~1200 batch checks and ~2600 single verifications). With the judge on,
 *   1. a rejected pass is searched breadth first with the same batch checks, from the root: while the failing nodes cover
 *      more than 16 proofs each and number at most search_width, both children of every failing node are checked and the
 *      failing ones kept; then every proof under a failing node is a suspect (search_width = 0: the whole pass);
 *   2. the proofs whose pi_b is outside the subgroup are suspects as well;
 *   3. when the call has at least judge_min suspects, each is decided by its OWN equation -- the single verifier's, no
 *      random scalar, a pi_b outside the subgroup judged as groth16_verify judges it -- one lane per suspect in launches of
 *      up to 65536 (judge_kernel of pairing.hip; the final exponentiation is code shared with the host, pairing.hpp). With
 *      fewer suspects they go to the single-proof verifier on the host, as with the judge off.
 * device < 0: the same policy with the judge on host threads. A key the batch refuses (a point off its curve, a G2 point
 * outside the subgroup) keeps its path: the single-proof verifier decides every proof.
 * Verdicts, the result code and error_msg are those of the judge-off call on the same inputs: the single verifier's.
 * judge = 0 is exactly the path of ug_groth16_verify_batch without ULTRAGROTH_VERIFY_JUDGE, stats included. */
typedef struct {
    unsigned size;                     /* sizeof(ug_verify_batch_options)                                              */
    int judge;                         /* 0 = off, 1 = on                                                              */
    int search_width;                  /* failing nodes the host search may hold per level; < 0: the library's (2)     */
    int judge_min;                     /* suspects of a call from which the judge decides them; < 0: the library's (256)*/
} ug_verify_batch_options;
typedef struct {
    ug_verify_batch_stats base;
    unsigned long long judged;         /* proofs decided by the judge                                                  */
    unsigned long long judge_launches; /* launches of judge_kernel (0 with device < 0)                                 */
    double judge_ms;                   /* wall time of the judge's device work, part of base.device_ms                 */
} ug_verify_batch_stats_ex;
/* options == NULL: as the calls above (the judge from the environment). */
int ug_groth16_verify_batch_opt(int device, int count, const char *const *proofs, const char *const *inputs,
                                const char *verification_key, int *verdicts, const ug_verify_batch_options *options,
                                ug_verify_batch_stats_ex *stats, char *error_msg, unsigned long error_msg_maxsize);
int ug_ultra_groth_verify_batch_opt(int device, int count, const char *const *proofs, const char *const *inputs,
                                    const char *verification_key, int *verdicts, const ug_verify_batch_options *options,
                                    ug_verify_batch_stats_ex *stats, char *error_msg, unsigned long error_msg_maxsize);

/* ---- packed proof records ------------------------------------------------------------------------------------------------
 * Services that verify in bulk hold proofs as fixed-size binary records; these calls take them as they are. A coordinate is
 * a plain (non-Montgomery) 256-bit little-endian integer of 32 bytes, in the order of proof.json:
 *   Groth16     pi_a.x, pi_a.y, pi_b.x.c0, pi_b.x.c1, pi_b.y.c0, pi_b.y.c1, pi_c.x, pi_c.y            256 bytes
 *   UltraGroth  pi_a (64) | pi_b (128) | pi_f (64) | pi_r (64)                                        320 bytes
 * and the public inputs of all proofs are count x n_pub x 32 contiguous bytes in the same integer form. A record STANDS FOR
 * the proof.json whose decimal strings are its integers (ug_proof_unpack writes that text), an input block for that
 * public.json: coordinates are taken mod q and inputs mod r as the JSON parsers take them, and (0, 0) is infinity. That is the
 * PLAIN layout; the _fmt calls below take two more.
 * verdicts[i] is what groth16_verify / ultra_groth_verify returns for the unpacked texts of record i, up to the 2^-128 of the
 * batch; a record cannot fail to parse, so it is VERIFIER_VALID_PROOF or VERIFIER_INVALID_PROOF. VERIFIER_ERROR, verdicts
 * untouched: null arguments or count < 0 ("null argument"), n_pub <= 0 ("invalid inputs data"), a key that does not parse,
 * n_pub + 1 != len(vk.IC) (the single call's length message), a device error. Options (NULL: the judge from the environment),
 * result code, error_msg and stats are those of the _opt calls; a key the batch refuses sends every proof to the single
 * verifier, as there.
 * device >= 0: the raw records of a pass of up to 65536 cross PCIe once. records_ingest_kernel (pairing.hip) reduces every
 * coordinate, sets the infinity flags, checks the curve equations and writes the arrays the Miller kernel reads; the
 * subgroup ladder answers for every pi_b in one launch (ug_points_check_mask's kernel); records that leave the batch -- a
 * point off its curve: INVALID; pi_b outside the subgroup: the single verifier or the judge -- are compacted away by a gather
 * kernel, and the Miller and tree kernels run on the resident arrays. The host draws the scalars, reduces the inputs and
 * keeps their prefix sums, derives the UltraGroth challenge from pi_r, makes the root check and the search; suspects are
 * rebuilt from their raw records. device < 0: the same protocol on host threads. */
int ug_groth16_verify_batch_records(int device, int count, const void *records, const void *inputs, int n_pub,
                                    const char *verification_key, int *verdicts, const ug_verify_batch_options *options,
                                    ug_verify_batch_stats_ex *stats, char *error_msg, unsigned long error_msg_maxsize);
int ug_ultra_groth_verify_batch_records(int device, int count, const void *records, const void *inputs, int n_pub,
                                        const char *verification_key, int *verdicts, const ug_verify_batch_options *options,
                                        ug_verify_batch_stats_ex *stats, char *error_msg, unsigned long error_msg_maxsize);

/* ---- record layouts ------------------------------------------------------------------------------------------------------
 * UG_RECORDS_PLAIN       the layout above.
 * UG_RECORDS_EVM         the same sizes, 256 / 320 bytes, in the order of the EVM pairing precompile's calldata: every 32-byte
 *                        coordinate is big-endian, and an Fq2 coordinate is stored imaginary part first, pi_b = x.c1, x.c0, y.c1,
 *                        y.c0. The input block is big-endian too. Everything else follows PLAIN: values are taken mod q / mod r,
 *                        and (0, 0) is infinity.
 * UG_RECORDS_COMPRESSED  one x coordinate and a sign bit per point: 128 bytes for Groth16 (pi_a 32 | pi_b 64 | pi_c 32), 160 for
 *                        UltraGroth (pi_a | pi_b | pi_f | pi_r). A G1 point is x as a 32-byte little-endian integer, a G2 point
 *                        x.c0 | x.c1, 64 bytes. The two top bits of the point's LAST byte are flags: bit 6 (0x40) means infinity --
 *                        the point is infinity whatever its other bits say -- and bit 7 (0x80) says that y is the larger of the two
 *                        roots, y > -y. For Fq "larger" means y > (q - 1) / 2 as an integer; for Fq2 c1 is compared first: if
 *                        c1 != 0, larger means c1 > (q - 1) / 2, and if c1 = 0 it means c0 > (q - 1) / 2. The remaining 254 bits
 *                        are x (for G2: of x.c1, with x.c0 a full word), taken mod q like every other coordinate here. The input
 *                        block is the PLAIN one.
 * A record of any layout STANDS FOR the plain record it converts to (ug_proof_record_convert), and through it for the proof.json
 * of ug_proof_unpack: its verdict is the single verifier's on that text, up to the batch's 2^-128. A compressed point whose x has
 * no y on the curve converts to nothing: such a record is VERIFIER_INVALID_PROOF, handled exactly like a point off its curve --
 * the same status and reason text, no pairing.
 * The _fmt calls are the records calls above with the layout as an argument; format = UG_RECORDS_PLAIN IS those calls, on the
 * same code path. An unknown format fails the call with VERIFIER_ERROR, "format: not one of UG_RECORDS_PLAIN, UG_RECORDS_EVM,
 * UG_RECORDS_COMPRESSED". device >= 0: the ingest kernel reads the layout itself -- EVM by loading a coordinate's words reversed,
 * COMPRESSED by taking the square roots in the lane that ingests the record (one Fq root per G1 point, up to three for pi_b:
 * fixed-exponent powers, pairing.hpp) -- and writes the same arrays, so everything after it is unchanged. The UltraGroth
 * challenge of a compressed record is derived from the pi_r the device decompressed; the host takes no root per proof. Suspects
 * and singles are rebuilt on the host from their raw records, those few only. device < 0: every record is converted on the host
 * threads. */
enum { UG_RECORDS_PLAIN = 0, UG_RECORDS_EVM = 1, UG_RECORDS_COMPRESSED = 2 };
/* bytes of one proof record: 256 / 320, or 128 / 160 compressed; 0 for an unknown format */
unsigned long ug_proof_record_bytes(int ultra, int format);
int ug_groth16_verify_batch_records_fmt(int device, int format, int count, const void *records, const void *inputs, int n_pub,
                                        const char *verification_key, int *verdicts, const ug_verify_batch_options *options,
                                        ug_verify_batch_stats_ex *stats, char *error_msg, unsigned long error_msg_maxsize);
int ug_ultra_groth_verify_batch_records_fmt(int device, int format, int count, const void *records, const void *inputs, int n_pub,
                                            const char *verification_key, int *verdicts, const ug_verify_batch_options *options,
                                            ug_verify_batch_stats_ex *stats, char *error_msg, unsigned long error_msg_maxsize);
/* ---- several keys in one call --------------------------------------------------------------------------------------------
 * A service that verifies proofs of many circuits pays the floor of a device pass -- one lane's Miller latency -- once per call,
 * so once per circuit with the calls above. The Miller loop of a proof does not read the key; only the end of a pass does. These
 * calls take n_keys key texts and key_of[count], the key of every proof, and make ONE device pass and ONE final exponentiation per
 * 65536 proofs, whatever the number of keys. One protocol per call: Groth16 and UltraGroth keys do not mix.
 *   verdicts[i] is what groth16_verify / ultra_groth_verify says of proof i under keys[key_of[i]], up to the batch's 2^-128. Proofs
 *   arrive in any order, interleaved between keys: the library groups them by key with a stable sort and answers in the caller's
 *   order; rc and error_msg follow the one-key rule, "proof <first bad index in the caller's order>: <reason>".
 *   The records calls take the layout as the _fmt calls do, and n_pub[n_keys], the inputs per proof of every key. Their input block
 *   is ragged: proof i owns n_pub[key_of[i]] x 32 bytes that start where proof i - 1's end, in the caller's order and the byte
 *   order of `format`.
 *   options and stats as the _opt calls; stats->ex is their struct. segments: the (pass, key) pairs that were batched; tree_launches:
 *   launches of the tree kernels (0 with device < 0), at most 2 ceil(log2(largest segment)) per pass; key_checks: the batch checks
 *   spent above the segments -- the one equation of every pass and the search over the keys --, part of ex.base.batch_checks.
 * VERIFIER_ERROR, verdicts untouched: an unknown format (the _fmt message); null arguments, count < 0 or n_keys < 0 ("null
 * argument"; key_of may be null when count == 0); n_keys <= 0 with count > 0; a key_of[i] outside [0, n_keys), "proof <i>: key index
 * <v> out of range"; n_pub[k] <= 0, "key <k>: invalid inputs data"; a key that does not parse, "key <k>: <the single call's
 * message>" -- keys that no proof names are parsed as well --; n_pub[k] + 1 != len(IC_k), "key <k>: <the length message>"; a device
 * error. count == 0 is valid.
 * A pass holds up to 65536 proofs in key order; the proofs of one key inside a pass are a SEGMENT, and a key whose proofs cross a
 * pass boundary has a segment in each. Scalars, prefix sums and vkX are per segment, as under one key; the trees are a forest,
 * one tree per segment, made by one launch per level for all segments. The pass is accepted by one equation, the product over its
 * segments of root_s e(-S_s alpha_s, beta_s) e(-vkX_s, gamma_s) e(-sum r C, delta_s) ..., and one final exponentiation. A pass that
 * fails is searched down a binary tree over its segments (both children of a failing node are checked, the failing ones entered),
 * then inside every failing segment as under one key, its root not checked again:
 *   batch_checks <= 1 + 2 (failing segments) ceil(log2 S) + sum over them of 2 bad_s ceil(log2(n_s / 16)),  single_checks <= 16 bad
 * for a pass of S segments. Judge on: the level of the keys follows the search_width rule of the proofs' level, and the suspects
 * of all keys are judged in ONE launch of up to 65536 (the keyed instantiation of judge_kernel; the cheap vkX step runs per key).
 * A key the batch refuses -- a point off its curve, a G2 point outside the subgroup -- sends ITS proofs to the single verifier;
 * the proofs under the other keys are batched as usual. n_keys == 1 gives the one-key call's verdicts, rc, message, batch_checks,
 * single_checks and off_subgroup on the same inputs, on the same code path: the one-key calls ARE this call with one key (a pass
 * of one segment keeps the one-key tree kernels and their tree layout, which the forest's is for one segment).
 * The keys are parsed and checked across the host threads. device < 0: the same protocol with the forest made on host threads. */
typedef struct {
    ug_verify_batch_stats_ex ex;
    unsigned long long segments, tree_launches, key_checks;
} ug_verify_batch_stats_keys;
int ug_groth16_verify_batch_keys(int device, int count, const char *const *proofs, const char *const *inputs, int n_keys,
                                 const char *const *keys, const int *key_of, int *verdicts, const ug_verify_batch_options *options,
                                 ug_verify_batch_stats_keys *stats, char *error_msg, unsigned long error_msg_maxsize);
int ug_ultra_groth_verify_batch_keys(int device, int count, const char *const *proofs, const char *const *inputs, int n_keys,
                                     const char *const *keys, const int *key_of, int *verdicts, const ug_verify_batch_options *options,
                                     ug_verify_batch_stats_keys *stats, char *error_msg, unsigned long error_msg_maxsize);
int ug_groth16_verify_batch_records_keys(int device, int format, int count, const void *records, const void *inputs, int n_keys,
                                         const char *const *keys, const int *key_of, const int *n_pub, int *verdicts,
                                         const ug_verify_batch_options *options, ug_verify_batch_stats_keys *stats, char *error_msg,
                                         unsigned long error_msg_maxsize);
int ug_ultra_groth_verify_batch_records_keys(int device, int format, int count, const void *records, const void *inputs, int n_keys,
                                             const char *const *keys, const int *key_of, const int *n_pub, int *verdicts,
                                             const ug_verify_batch_options *options, ug_verify_batch_stats_keys *stats,
                                             char *error_msg, unsigned long error_msg_maxsize);

/* One record from one layout to another, every coordinate reduced mod q on the way (from == to: the record reduced). 0 = converted;
 * 1 = the source holds no point to convert -- from COMPRESSED an x with no root, to COMPRESSED a point that is not on its curve,
 * since a sign bit cannot stand for it; 2 = a null argument or an unknown format. `to` is written only on 0. PLAIN <-> EVM never
 * returns 1, and COMPRESSED -> PLAIN of PLAIN -> COMPRESSED of a record is that record with every coordinate reduced. */
int ug_proof_record_convert(int ultra, int from_format, const void *from, int to_format, void *to);
/* One proof's input block, n_pub x 32 bytes, from the byte order of one layout to that of another: a byte reversal of every value
 * between EVM and the other two, else a copy; values are not reduced. 0 = ok; 2 = a null argument, n_pub <= 0 or an unknown format. */
int ug_inputs_convert(int from_format, const void *from, int n_pub, int to_format, void *to);

/* proof.json -> record (256 / 320 bytes). 0 = ok; 1 = the text does not parse as a proof of that protocol, or a value is >= 2^256 */
int ug_proof_pack(int ultra, const char *proof_json, void *record);
/* public.json -> n_pub x 32 bytes. 0 = ok; 1 = parse error, a value >= 2^256 or another count than n_pub */
int ug_inputs_pack(const char *inputs_json, void *out, int n_pub);
/* the text a record / an input block stands for, NUL-terminated. 0 = ok; 1 = maxsize is too small (1100 bytes hold any Groth16
 * record, 1400 any UltraGroth record, 81 * n_pub + 3 any input block) or a null argument */
int ug_proof_unpack(int ultra, const void *record, char *json, unsigned long maxsize);
int ug_inputs_unpack(const void *in, int n_pub, char *json, unsigned long maxsize);

/* milliseconds of the last device pass of this process: miller_batch_kernel, the Fq12 tree, the G1 tree */
void ug_verify_batch_kernel_ms(double ms[3]);
/* where the wall time of the last batch call of this process went, in milliseconds:
 *   [0] the key   [1] step 1: parsing the texts, the curve checks (records on a device: the inputs and the challenge only)
 *   [2] step 2: the pi_b as records and the subgroup check (records on a device: upload, ingest kernel, ladder, status bytes)
 *   [3] the scalars, the inputs times the scalars, the prefix sums   [4] packing the word arrays (none for resident records)
 *   [5] the pass: uploads, the three kernels (ug_verify_batch_kernel_ms), the trees' download
 *   [6] the root check and the search   [7] the judge and the single verifier */
void ug_verify_batch_phase_ms(double ms[8]);

/* Test hooks, live only in a process started with ULTRAGROTH_TEST_HOOKS=1 (else they return 1 and write nothing).
 * ug_test_verify_batch_trace: for proof `index` of the last batch call, if it was batched, its scalar r (128 bits) and
 * f = miller(pi_b, r pi_a) as 12 x 9 limbs of 29 bits (canonical, Montgomery radix 2^261). ug_test_miller: the host's
 * Miller loop of one pair given as zkey records (Montgomery radix 2^256), in the same form. ug_test_final_exp: the final
 * exponentiation's is-one test of f in that form -- g = (f^(p^2) f)^((p^4 - p^2 + 1)/r), the value after the hard part, and
 * *is_one = whether f^((p^12 - 1)/r) is 1 -- on the host for device < 0, else by a one-lane launch of the device code. */
int ug_test_verify_batch_trace(int index, unsigned int scalar[4], unsigned int f[108]);
int ug_test_miller(const unsigned char g1[64], const unsigned char g2[128], unsigned int f[108]);
int ug_test_final_exp(int device, const unsigned int f[108], unsigned int g[108], int *is_one);
/* the passes of the last records call on a device: [0] those that used the resident arrays in place, [1] those that compacted
 * them through the gather kernel first */
int ug_test_verify_records_passes(unsigned long long passes[2]);
/* Upload and ingest only, count records of `format`: plain_out gets, per record, the plain 256 / 320 bytes that the device's arrays
 * hold afterwards -- coordinates reduced, infinity as zeros, a point that failed (no root, off its curve) as zeros -- and status the
 * record's UG_POINT_* byte. device < 0: the host's reading of the same records. */
int ug_test_records_ingest(int device, int format, int ultra, int count, const void *records, void *plain_out, unsigned char *status);
/* f2_sqrt (pairing.hpp) of count values, each 64 bytes plain little-endian c0 | c1: out gets the root that is NOT the larger one in
 * the same form (zeros when there is none), has_root one byte each. One lane per element on a device; device < 0: the host's code. */
int ug_test_fq2_sqrt(int device, int count, const void *in, void *out, unsigned char *has_root);
/* Only the trees over given leaves: n_segments segments of sizes[] leaves each (n in all, at most 65536), leaves_f n x 108 words
 * and leaves_g n x k x 36 words as the Miller kernel leaves them (canonical limbs; k = 1 or 2 G1 sums per proof). The forest
 * kernels make them on `device`; device < 0: the host forest. f_tree_out / g_tree_out get the whole forest, nodes x 108 and
 * nodes x k x 36 words: level 0 is the leaves; level l + 1 holds, in segment order, the (m + 1) / 2 nodes of every segment that has
 * m > 1 nodes on level l (one segment: the tree of a one-key pass). Values are canonical, so both agree byte for byte. */
int ug_test_tree_forest(int device, int k, int n_segments, const int *sizes, const unsigned int *leaves_f, const unsigned int *leaves_g,
                        unsigned int *f_tree_out, unsigned int *g_tree_out);

#ifdef __cplusplus
}
#endif
#endif
