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
 * public.json: coordinates are taken mod q and inputs mod r as the JSON parsers take them, and (0, 0) is infinity. Other
 * byte orders (EVM calldata) are the caller's to convert.
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

#ifdef __cplusplus
}
#endif
#endif
