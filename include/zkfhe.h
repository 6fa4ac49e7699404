/* zkfhe.h -- C ABI of the MI355X (gfx950) backend for zk-fhe's BFV-proof hot path.
 *
 * The reference (enricobottazzi/zk-fhe) is a Rust crate with no FFI of its own; its prover hot loops
 * live in third-party crates reached through the single call `run_eth(bfv_encryption_circuit, args)`
 * (reference examples/bfv.rs:311).  Each entry point below names the Rust seam it replaces -- the
 * function a maintainer would re-route through `extern "C"` (binding stubs: INTEGRATION.md):
 *
 *   zkfhe_ntt_batch        <- halo2_proofs::arithmetic::best_fft(&mut [Fr], omega, log_n) and
 *                             poly::EvaluationDomain::{lagrange_to_coeff, coeff_to_lagrange}
 *   zkfhe_coset_ntt_batch  <- EvaluationDomain::{coeff_to_extended, extended_to_coeff}
 *   zkfhe_g1_fft           <- best_fft::<G1> as g_to_lagrange uses it (ParamsKZG::downsize: zkfhe_srs_load_downsized)
 *   zkfhe_basis_create     <- poly::kzg::commitment::ParamsKZG {g, g_lagrange} (the SRS halves)
 *   zkfhe_msm_batch        <- arithmetic::best_multiexp(&[Fr], &[G1Affine]) as used by
 *                             ParamsKZG::{commit, commit_lagrange}
 *   zkfhe_fr_*             <- the coefficient-wise Fr mul/add/sub loops of `parallelize(...)` bodies
 *                             (and src/poly_chip.rs:122-174 add / scalar_mul witness values)
 *   zkfhe_fr_batch_invert  <- ff::BatchInvert / halo2 `batch_invert_assigned`
 *   zkfhe_witness_*        <- the per-coefficient witness loops of src/poly_chip.rs:226-252
 *                             (reduce_by_modulo -> RangeChip::div_mod) and src/poly.rs:75-191
 *
 * Data layouts (identical to halo2curves' in-memory representation):
 *   Fr, Fq      4 x uint64_t little-endian limbs, Montgomery form with R = 2^256, value < p.
 *   G1 affine   {Fq x, Fq y} = 64 bytes; the identity is (0, 0).
 * Conventions: every call returns 0 on success or a negative ZKFHE_E* code and never throws or aborts
 * across the ABI; zkfhe_last_error() gives the message.  `*_dev` pointers are device (HBM) addresses
 * obtained from zkfhe_dev_alloc (or any hipMalloc'd buffer of the same process); everything else is
 * host memory.  One context per GPU; calls on one context are ordered on its stream and are
 * asynchronous with respect to the host unless stated (zkfhe_sync / zkfhe_download wait).
 * There is no CPU fallback: without the HIP runtime and a gfx950 device zkfhe_ctx_create fails.
 */
#ifndef ZKFHE_H
#define ZKFHE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKFHE_OK 0
#define ZKFHE_EINVAL (-1)   /* bad argument */
#define ZKFHE_EHIP (-2)     /* HIP runtime error (message in zkfhe_last_error) */
#define ZKFHE_ENOMEM (-3)
#define ZKFHE_ENODEV (-4)   /* no usable gfx950 device */

typedef struct zkfhe_ctx zkfhe_ctx;
typedef struct zkfhe_basis zkfhe_basis;

typedef struct { uint64_t l[4]; } zkfhe_fr;
typedef struct { uint64_t l[4]; } zkfhe_fq;
typedef struct { zkfhe_fq x, y; } zkfhe_g1_affine;
/* accumulator form of a G1 point (EFD "XYZZ"): x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2; the identity has ZZ = ZZZ = 0.  128 bytes,
 * raw Montgomery coordinates.  What an MSM holds before its one field inversion. */
typedef struct { zkfhe_fq x, y, zz, zzz; } zkfhe_g1_xyzz;

/* ---- context / memory -------------------------------------------------------------------- */
/* hip_stream: an existing hipStream_t to run on, or NULL to let the context create its own. */
int zkfhe_ctx_create(int device_id, void *hip_stream, zkfhe_ctx **out);
int zkfhe_ctx_destroy(zkfhe_ctx *ctx);
const char *zkfhe_last_error(const zkfhe_ctx *ctx);   /* ctx may be NULL: last creation error */
int zkfhe_sync(zkfhe_ctx *ctx);
void *zkfhe_stream(zkfhe_ctx *ctx);                   /* the hipStream_t the context launches on */
int zkfhe_device_info(zkfhe_ctx *ctx, char *arch_name, size_t arch_len, int *num_cu, size_t *hbm_bytes);

int zkfhe_dev_alloc(zkfhe_ctx *ctx, size_t bytes, void **dptr);
int zkfhe_dev_free(zkfhe_ctx *ctx, void *dptr);
int zkfhe_upload(zkfhe_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);     /* waits */
int zkfhe_download(zkfhe_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);   /* waits */
int zkfhe_copy_dev(zkfhe_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);
int zkfhe_memset_dev(zkfhe_ctx *ctx, void *dst_dev, int byte, size_t bytes);

/* HIP-event timing on the context's stream (what bench.py uses for per-kernel durations). */
int zkfhe_timer_start(zkfhe_ctx *ctx);
int zkfhe_timer_stop_ms(zkfhe_ctx *ctx, float *ms);   /* waits for the stop event */

/* Per-kernel profiling with HIP events on the context's stream.  While enabled, zkfhe_msm_batch and
 * zkfhe_ntt_batch bracket their dominant kernel (which 0: the summing kernel of a wide MSM call -- k_msm_table or k_msm_accumulate --, 1: the NTT tile kernel (k_ntt13 at n >= 2^13),
 * 2: k_msm_table of a call of a few columns) with an event pair
 * and wait for it, accumulating duration, launch count and ALGORITHMIC bytes (MSM: 96 B per term, NTT: 64 B per
 * point -- BASELINE.md).  Meant for a separate, untimed pass (it serialises the stream). */
int zkfhe_prof_enable(zkfhe_ctx *ctx, int on);
int zkfhe_prof_reset(zkfhe_ctx *ctx);
int zkfhe_prof_read(zkfhe_ctx *ctx, int which, double *total_ms, uint64_t *launches, double *algorithmic_bytes);
/* further slots of zkfhe_prof_read: the batch verifier's kernels (algorithmic bytes: 32 B in per point; 96 B per MSM term) */
#define ZKFHE_PROF_G1_DECOMPRESS 3   /* k_g1_decompress */
#define ZKFHE_PROF_MSM_SEGMENTED 4   /* k_msm_segmented */
/* arithmetic units of the profiled launches: which = 0 -> mixed point additions (k_msm_accumulate), 1 -> butterflies (NTT tile kernel) */
int zkfhe_prof_read_ops(zkfhe_ctx *ctx, int which, double *ops);

/* Host-side marks of the LAST zkfhe_bfv_prove on this context, in ms from its start: [0] the phase-0 commitment is back from the
 * GPU (what the transcript absorbs next), [1] the first challenge is squeezed -- it stands behind the sponge over the public
 * inputs (examples/bfv.rs:118-122: 5 N + 1 values, one sequential Poseidon chain with the reference's transcript), so [1] - [0]
 * is the time a lone proof waits for the HOST --, [2] the proof is complete. */
int zkfhe_ctx_last_proof_marks(zkfhe_ctx *ctx, float marks_ms[3]);
/* Commands the LAST zkfhe_bfv_prove / zkfhe_bfv_prove_words on this context put on its streams (the auxiliary stream of its
 * workspace included), counted on the host where the library issues them: [0] kernel launches, [1] copy commands
 * (hipMemcpy*Async), [2] fill commands (hipMemsetAsync).  Reset when a proof starts; costs nothing on the GPU. */
int zkfhe_ctx_last_proof_commands(zkfhe_ctx *ctx, uint64_t counts[3]);

/* ---- coefficient-wise Fr arithmetic (device buffers, out may alias a or b) ----------------- */
int zkfhe_fr_add(zkfhe_ctx *ctx, const zkfhe_fr *a_dev, const zkfhe_fr *b_dev, zkfhe_fr *out_dev, size_t n);
int zkfhe_fr_sub(zkfhe_ctx *ctx, const zkfhe_fr *a_dev, const zkfhe_fr *b_dev, zkfhe_fr *out_dev, size_t n);
int zkfhe_fr_mul(zkfhe_ctx *ctx, const zkfhe_fr *a_dev, const zkfhe_fr *b_dev, zkfhe_fr *out_dev, size_t n);
/* out[i] = a[i] * s   (s: one host-side Fr) */
int zkfhe_fr_scale(zkfhe_ctx *ctx, const zkfhe_fr *a_dev, const zkfhe_fr *s_host, zkfhe_fr *out_dev, size_t n);
/* canonical integer <-> Montgomery form */
int zkfhe_fr_to_mont(zkfhe_ctx *ctx, const zkfhe_fr *a_dev, zkfhe_fr *out_dev, size_t n);
int zkfhe_fr_from_mont(zkfhe_ctx *ctx, const zkfhe_fr *a_dev, zkfhe_fr *out_dev, size_t n);
/* in place a[i] <- a[i]^-1, zero stays zero (halo2 batch_invert convention) */
int zkfhe_fr_batch_invert(zkfhe_ctx *ctx, zkfhe_fr *a_dev, size_t n);
/* the same inversion with a numerator: num[i] <- num[i] * den[i]^-1 in one kernel (0 where den[i] = 0: what the call above followed
 * by zkfhe_fr_mul gives); den is only read and must not alias num */
int zkfhe_fr_batch_invert_mul(zkfhe_ctx *ctx, const zkfhe_fr *den_dev, zkfhe_fr *num_dev, size_t n);
/* The nine-limb Fr arithmetic of the prover's kernels, element by element (a test entry).  in_dev holds five operand arrays of n
 * elements one after the other (a, b, c, d, e; an operation reads the ones it names), out_dev n results, canonical.
 * op 0: a b;  1: a^2;  2: a b + c d;  3: a (b + c d + e), a step of a permutation product;  4: (a + b)(c + d), a lookup term;
 * 5: a b c, the first product regrouped in registers as the constant operand of the second. */
int zkfhe_fr9_op(zkfhe_ctx *ctx, int op, const zkfhe_fr *in_dev, zkfhe_fr *out_dev, size_t n);
/* modmul micro-benchmark: out[i] = a[i]^(2^iters) by repeated squaring (ALU-roofline probe) */
int zkfhe_fr_sqr_chain(zkfhe_ctx *ctx, const zkfhe_fr *a_dev, zkfhe_fr *out_dev, size_t n, int iters);
/* the same probe for the radix-2^29 product the MSM kernels use (nine 29-bit limbs, Montgomery constant 2^261): a[i] < q as a
 * packed 256-bit integer, out[i] = a[i]^(2^iters) * (2^-261)^(2^iters - 1) mod q, canonical */
int zkfhe_fq29_sqr_chain(zkfhe_ctx *ctx, const zkfhe_fq *a_dev, zkfhe_fq *out_dev, size_t n, int iters);

/* ---- NTT ---------------------------------------------------------------------------------- */
/* n_cols independent transforms of length 2^log_n, column c at cols_dev + c * 2^log_n, in place,
 * natural order in and out.  inverse = 0: out[i] = sum_j a[j] w^(ij) with w = halo2's omega for
 * this log_n (= ROOT_OF_UNITY^(2^(28-log_n)));  inverse = 1: w^-1 and a final multiplication by
 * n^-1 (lagrange_to_coeff).  1 <= log_n <= 26. */
int zkfhe_ntt_batch(zkfhe_ctx *ctx, zkfhe_fr *cols_dev, size_t n_cols, int log_n, int inverse);
/* The same transform out of place (in_dev and out_dev distinct, not overlapping): EvaluationDomain::lagrange_to_coeff /
 * coeff_to_lagrange consume one Polynomial and return another.  This is the form the kernels run natively at n = 2^13 (two
 * workgroups per column, each reading all of it): the in-place call above goes through a scratch copy there. */
int zkfhe_ntt_batch_to(zkfhe_ctx *ctx, const zkfhe_fr *in_dev, zkfhe_fr *out_dev, size_t n_cols, int log_n, int inverse);

/* coeff_to_extended (inverse = 0): column c holds 2^log_n coefficients at in_dev + c*2^log_n; writes
 * the 2^(log_n+log_ext_factor) evaluations over the coset g*<w_ext> to out_dev + c*2^(log_n+lef) in
 * COSET-MAJOR order: out[k1*2^log_n + k2] = f(g * w_ext^(k1 + 2^lef * k2)), i.e. row k1 is the
 * evaluation over (g*w_ext^k1)*<w>; a rotation by w stays inside a row.
 * extended_to_coeff (inverse = 1): the same layout in -> 2^(log_n+lef) coefficients out (natural order).
 * g is `zeta`-coset generator of halo2's extended domain, passed by the caller (host Fr). */
int zkfhe_coset_ntt_batch(zkfhe_ctx *ctx, const zkfhe_fr *in_dev, zkfhe_fr *out_dev, size_t n_cols,
                          int log_n, int log_ext_factor, const zkfhe_fr *g_host, int inverse);

/* ---- MSM (KZG commit) ---------------------------------------------------------------------- */
/* Uploads n affine bases (host memory) and builds the per-window tables 2^(c*w) * P_i used by the
 * single-bucket-set Pippenger (DESIGN.md "MSM").  window_bits = 0 picks the default for n. */
int zkfhe_basis_create(zkfhe_ctx *ctx, const zkfhe_g1_affine *bases_host, size_t n, int window_bits,
                       zkfhe_basis **out);
int zkfhe_basis_destroy(zkfhe_ctx *ctx, zkfhe_basis *basis);
size_t zkfhe_basis_len(const zkfhe_basis *basis);
/* out_dev[c] = sum_i scalars_dev[c*n + i] * bases[i], c < n_cols; n = zkfhe_basis_len; result affine */
int zkfhe_msm_batch(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_fr *scalars_dev, size_t n_cols,
                    zkfhe_g1_affine *out_dev);

/* A few non-zero scalars against a basis (one with a digit-multiple table: zkfhe_basis_has_multiples; n <= 2^16, default
 * window bits): out_dev[slot] = sum of scalar * P_row over the terms of that slot, slot < n_slots.  scalar: Montgomery Fr.
 * One wave per slot -- the right tool when a column is all zero except a handful of cells. */
typedef struct { zkfhe_fr scalar; uint32_t row; uint32_t slot; } zkfhe_sparse_term;
int zkfhe_msm_sparse(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_sparse_term *terms_dev, size_t n_terms, size_t n_slots,
                     zkfhe_g1_affine *out_dev);
/* The same two calls with the sums left in the accumulator form: the call's last kernel skips its field inversion (a 40 us
 * dependent chain in one lane at the end of every call) and the caller normalises many points with ONE inversion on the host --
 * what halo2's create_proof does with a round's commitments (`commit_lagrange` returns projective points, the round is
 * batch-normalised: SURVEY.md Appendix B step 2).  out_dev may be pinned host memory, like every *_dev output of this header.
 * zkfhe_g1_xyzz_to_affine runs on the calling thread (no device work): Montgomery's trick over the ZZZ, one inversion for the
 * array; in / out are host pointers and must not overlap. */
int zkfhe_msm_batch_xyzz(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_fr *scalars_dev, size_t n_cols,
                         zkfhe_g1_xyzz *out_dev);
int zkfhe_msm_sparse_xyzz(zkfhe_ctx *ctx, const zkfhe_basis *basis, const zkfhe_sparse_term *terms_dev, size_t n_terms, size_t n_slots,
                          zkfhe_g1_xyzz *out_dev);
int zkfhe_g1_xyzz_to_affine(const zkfhe_g1_xyzz *in, size_t n, zkfhe_g1_affine *out);
int zkfhe_basis_has_multiples(const zkfhe_basis *basis);
/* Digit width of the basis' digit-multiple table (0: none).  *wide_calls (optional) = 1 when calls of many columns take the
 * table path too (k_msm_table), 0 when they take the bucket pipeline (k_msm_accumulate ...) and only calls of <= 8 columns
 * go through the table. */
int zkfhe_basis_table_bits(const zkfhe_basis *basis, int *wide_calls);
/* Resident bytes of that table; *narrowed (optional) = 1 when it is narrower than its budget allowed because the device did not
 * have the room when the basis was made (ZKFHE_TABLE_GB: default 48 and at most a quarter of the free memory; a reserve of an
 * eighth of the device, at least 24 GB, always stays free for keys and workspaces -- ZKFHE_TABLE_RESERVE_GB). */
size_t zkfhe_basis_table_bytes(const zkfhe_basis *basis, int *narrowed);

/* ---- intra-proof multi-GPU: commitments sharded by point range (replaces nothing in the reference,
 * whose prover is single-process -- the seam is again best_multiexp inside ParamsKZG::{commit, commit_lagrange}) ----------
 * One process per GPU.  Rank r of W owns the bases [n r / W, n (r+1) / W) of each SRS half and the same rows of every
 * column; zkfhe_msm_batch_sharded computes its partial sums, all-gathers the 64-byte affine partials as raw bytes
 * (ncclAllGather of ncclUint8 over RCCL / xGMI, on the context's stream) and adds them on every rank, so all ranks hold the
 * same commitments, the same transcript and the same proof bytes as a single GPU.  An SRS made with
 * zkfhe_srs_create_sharded carries the communicator: zkfhe_bfv_keygen / zkfhe_bfv_prove then shard every commitment with
 * no further change (every rank calls them with the same inputs and seed).
 * zkfhe_comm_create needs librccl.so at run time (dlopen; nothing is linked).  zkfhe_comm_create_with_transport takes a host
 * all-gather callback instead (MPI, gloo, a test shim): recv = the `world` send buffers of `bytes` bytes each, rank-major;
 * return 0 on success. */
typedef struct zkfhe_comm zkfhe_comm;
typedef int (*zkfhe_allgather_fn)(void *user, const void *send, size_t bytes, void *recv);
int zkfhe_comm_unique_id(uint8_t id_out[128]);   /* rank 0: ncclGetUniqueId, to be passed to the other ranks out of band */
int zkfhe_comm_create(zkfhe_ctx *ctx, int rank, int world, const uint8_t unique_id[128], zkfhe_comm **out);
int zkfhe_comm_create_with_transport(zkfhe_ctx *ctx, int rank, int world, zkfhe_allgather_fn allgather, void *user, zkfhe_comm **out);
int zkfhe_comm_destroy(zkfhe_ctx *ctx, zkfhe_comm *comm);
int zkfhe_comm_rank(const zkfhe_comm *comm);
int zkfhe_comm_world(const zkfhe_comm *comm);
/* non-zero when commitments made with this communicator go through a collective: world > 1, or a one-rank RCCL communicator */
int zkfhe_comm_active(const zkfhe_comm *comm);
void zkfhe_comm_point_range(const zkfhe_comm *comm, size_t n, size_t *lo, size_t *hi);
int zkfhe_comm_all_gather(zkfhe_ctx *ctx, zkfhe_comm *comm, const void *send_dev, void *recv_dev, size_t bytes);
/* The same collective on the communicator's own stream (RCCL and one-rank communicators; the callback transport completes on the
 * context's stream as zkfhe_comm_all_gather does): it starts behind everything queued on the context's stream so far and overlaps
 * what is queued there next; zkfhe_comm_join orders the context's stream or the caller behind it.  Both buffers stay untouched
 * until then. */
int zkfhe_comm_all_gather_async(zkfhe_ctx *ctx, zkfhe_comm *comm, const void *send_dev, void *recv_dev, size_t bytes);
/* basis_slice: a basis made of this rank's point range; column c's scalars for that range at scalars_dev + c * col_stride
 * (col_stride = the full column length when scalars_dev points at row lo of column 0).  out_dev[c]: the full MSM, on every rank. */
int zkfhe_msm_batch_sharded(zkfhe_ctx *ctx, zkfhe_comm *comm, const zkfhe_basis *basis_slice, const zkfhe_fr *scalars_dev,
                            size_t col_stride, size_t n_cols, zkfhe_g1_affine *out_dev);
/* The same with the collective off the context's stream: the partial MSM runs on the context's stream, the all-gather and the sum
 * on the communicator's own, so kernels queued on the context's stream after the call (the next batch's partial MSM, witness
 * kernels) overlap the exchange over xGMI.  out_dev is complete after zkfhe_comm_join: block_host = 0 makes the context's stream
 * wait for every collective queued so far, 1 the calling thread.  zkfhe_comm_record_event records a HIP event (hipEvent_t)
 * behind them instead.  With a callback transport (host all-gather) the call completes on the context's stream like
 * zkfhe_msm_batch_sharded and the join is a plain wait.  Every rank must issue these calls in the same order. */
int zkfhe_msm_batch_sharded_async(zkfhe_ctx *ctx, zkfhe_comm *comm, const zkfhe_basis *basis_slice, const zkfhe_fr *scalars_dev, size_t col_stride,
                                  size_t n_cols, zkfhe_g1_affine *out_dev);
int zkfhe_comm_join(zkfhe_ctx *ctx, zkfhe_comm *comm, int block_host);
int zkfhe_comm_record_event(zkfhe_ctx *ctx, zkfhe_comm *comm, void *hip_event);

/* ---- G1 helpers (device, used by tests and by the SRS builder) ------------------------------ */
/* out[i] = a[i] + b[i] (affine in, affine out; handles doubling / inverse / identity) */
int zkfhe_g1_add(zkfhe_ctx *ctx, const zkfhe_g1_affine *a_dev, const zkfhe_g1_affine *b_dev,
                 zkfhe_g1_affine *out_dev, size_t n);
/* out[i] = k[i] * p[i] */
int zkfhe_g1_mul(zkfhe_ctx *ctx, const zkfhe_g1_affine *p_dev, const zkfhe_fr *k_dev,
                 zkfhe_g1_affine *out_dev, size_t n);
/* halo2 best_fft::<G1> / g_to_lagrange.  points_dev: 2^log_n affine points, Montgomery limbs, identity = (0, 0); in place,
 * natural order in and out.  inverse == 0: out[i] = sum_j w^(ij) P_j.  inverse != 0: out[i] = n^-1 sum_j w^(-ij) P_j.
 * w = the 2^log_n-th root of zkfhe_ntt_batch.  1 <= log_n <= 20.  Waits.
 * Any points on the curve are taken: equal, opposite and identity summands go through the complete addition.  Between the stages
 * the points stay in the accumulator form in the context's scratch (128 B x 2^log_n, and 256 B x 2^log_n of window tables); one
 * field inversion per point at the end. */
int zkfhe_g1_fft(zkfhe_ctx *ctx, zkfhe_g1_affine *points_dev, int log_n, int inverse);
#define ZKFHE_PROF_G1_FFT 23   /* k_g1_fft_shared, k_g1_fft_window: 256 B per point and stage; ops = scalar multiplications */
/* Decompression of n 32-byte compressed G1 points (the proof byte stream's form: x little-endian, the sign and identity bits of
 * byte 31 as ZKFHE_POINT_ENCODING selects) into Montgomery affine points, identity = (0, 0), with one status per point.  Any bytes
 * are accepted; a point whose status is not ZKFHE_PT_OK is written as (0, 0).  The same checks, in the same order, as the host
 * verifier's reader.  halo2curves: G1Affine::from_bytes. */
#define ZKFHE_PT_OK 0
#define ZKFHE_PT_X_NOT_REDUCED 1   /* x >= q */
#define ZKFHE_PT_NOT_ON_CURVE 2    /* x^3 + 3 is not a square */
#define ZKFHE_PT_BAD_IDENTITY 3    /* the identity bit with any other bit set */
int zkfhe_g1_decompress(zkfhe_ctx *ctx, const uint8_t *in_dev, size_t n, zkfhe_g1_affine *out_dev, int32_t *status_dev);
/* Many small MSMs over one array of affine points addressed by index (halo2 MSM::eval of many snarks' openings at once):
 *   out[s] = sum over t in [seg_off[s], seg_off[s+1]) of scalars[t] * points[index[t]],  s < n_segs
 * scalars: n_terms Montgomery Fr; seg_off: n_segs + 1 ascending offsets into [0, n_terms]; index: n_terms values < n_points.
 * Segments may be empty (identity), repeat indices, hold zero scalars or identity points.  One workgroup per segment: meant for
 * segments of up to a few thousand terms (the wide MSMs of the prover are zkfhe_msm_batch).  Waits for the result; a bad index
 * or offset is ZKFHE_EINVAL (out_dev then undefined). */
int zkfhe_msm_segmented(zkfhe_ctx *ctx, const zkfhe_g1_affine *points_dev, size_t n_points, const uint32_t *index_dev,
                        const zkfhe_fr *scalars_dev, size_t n_terms, const uint32_t *seg_off_dev, size_t n_segs,
                        zkfhe_g1_affine *out_dev);

/* ---- BFV witness kernels -------------------------------- */
/* Negacyclic product in R_q = Z_q[x]/(x^N+1) is NOT what the reference computes: Poly::mul
 * (src/poly.rs:75-103) is the plain integer product of two degree-(N-1) polynomials, 2N-1 coefficients.
 * a, b: N canonical integers < 2^64 each (uint64), big-endian coefficient order as in bfv.in;
 * out: 2N-1 Montgomery Fr values (exact integers, < 2^132 << r).  N a power of two <= 2^20. */
int zkfhe_witness_poly_mul_u64(zkfhe_ctx *ctx, const uint64_t *a_dev, const uint64_t *b_dev, size_t n,
                               zkfhe_fr *out_dev);
/* The same product on the host for short, narrow polynomials (n a power of two <= 2048, every coefficient below 2^32: the
 * k = 13 circuit's pk_i * u): an exact NTT convolution over p = 2^64 - 2^32 + 1 on one core (host/poly_ntt64.hpp), which is
 * what Poly::mul uses for them inside zkfhe_bfv_prove.  lo / hi: 2n - 1 coefficients as 128-bit integers.  ZKFHE_EINVAL when
 * the operands do not fit. */
int zkfhe_host_poly_mul_u32(const uint64_t *a, const uint64_t *b, size_t n, uint64_t *lo, uint64_t *hi);
/* RangeChip::div_mod witness (src/poly_chip.rs:236-246): for canonical values a[i] < 2^128 held as
 * Montgomery Fr, q a u64 modulus: div[i] = floor(a/q), rem[i] = a mod q (both returned as Montgomery Fr). */
int zkfhe_witness_div_mod(zkfhe_ctx *ctx, const zkfhe_fr *a_dev, uint64_t q, zkfhe_fr *div_dev,
                          zkfhe_fr *rem_dev, size_t n);

/* ---- Fiat-Shamir transcript (host only; replaces snark-verifier `PoseidonTranscript<NativeLoader>` /
 * halo2_proofs `Blake2bWrite`, reached from reference examples/bfv.rs:311 via gen_snark_shplonk) -------------- */
#define ZKFHE_TRANSCRIPT_POSEIDON 0   /* T = 3, RATE = 2, R_F = 8, R_P = 57 over BN254 Fr: what the reference proves / verifies with */
#define ZKFHE_TRANSCRIPT_BLAKE2B 1    /* halo2's "Halo2-Transcript" Blake2b with Challenge255 */
typedef struct zkfhe_transcript zkfhe_transcript;
int zkfhe_transcript_create(uint32_t kind, zkfhe_transcript **out);
void zkfhe_transcript_destroy(zkfhe_transcript *t);
/* scalars: canonical 32-byte little-endian Fr; points: canonical affine x || y (64 bytes, little-endian Fq each).
 * common_* only absorb; write_* also append the 32-byte encoding to the byte stream: a scalar as it is, a point as halo2curves'
 * bn256 G1Affine::to_bytes -- x little-endian, (y & 1) << 6 in byte 31, the identity as 0x80 in byte 31 and zeros. */
int zkfhe_transcript_common_scalar(zkfhe_transcript *t, const uint8_t s_le[32]);
int zkfhe_transcript_write_scalar(zkfhe_transcript *t, const uint8_t s_le[32]);
int zkfhe_transcript_common_point(zkfhe_transcript *t, const uint8_t xy_le[64]);
int zkfhe_transcript_write_point(zkfhe_transcript *t, const uint8_t xy_le[64]);
int zkfhe_transcript_squeeze(zkfhe_transcript *t, uint8_t challenge_le[32]);
int zkfhe_transcript_bytes(const zkfhe_transcript *t, uint8_t *out, size_t cap, size_t *len);
/* The Poseidon instance itself: one permutation of three canonical 32-byte LE words in place, and the generated
 * constants (65 x 3 round constants, 3 x 3 MDS, canonical 32-byte LE each) for cross-checks. */
int zkfhe_poseidon_permute(uint8_t state_le[96]);
int zkfhe_poseidon_constants(uint8_t round_constants_le[65 * 3 * 32], uint8_t mds_le[9 * 32]);
/* n_jobs independent sponge hashes (fresh sponge, absorb counts[j] canonical scalars taken in order from values_le, squeeze) --
 * the parity and timing hook of the eight-lane sponge engine the prover's transcripts share when several proofs are in flight
 * (host/poseidon_x8.cpp: one sponge per AVX-512 IFMA lane, ragged lengths, lanes refilled as they run dry).
 * mode 0: the scalar / single-sponge path (what a lone transcript runs); 1: eight lanes on the calling thread; 2: through the
 * hash service's worker threads, as the prover does.  Modes 1 and 2 return ZKFHE_ENODEV on a CPU without AVX-512 IFMA.
 * No GPU involved; the same digests in every mode. */
/* How the Poseidon transcripts of the proofs in flight in this process hash: 0 = every transcript on its own (lowest latency:
 * the default), 1 = long runs of all of them through the shared eight-lane service (about half the host CPU per proof, about
 * twice the hashing latency: for hosts with few CPUs per GPU), -1 = query.  Returns the mode in force (ZKFHE_EINVAL for any
 * other argument).  Process-wide; takes effect for transcripts' next runs.  Initial value from ZKFHE_HASH_MODE=latency|shared. */
int zkfhe_host_hash_mode(int mode);
int zkfhe_poseidon_hash_many(const uint8_t *values_le, const size_t *counts, size_t n_jobs, int mode, uint8_t *digests_le);

/* ---- BFV circuit: witness tables, keygen, prove (reference examples/bfv.rs + halo2-scaffold run_eth) ---- */
/* Runtime form of the compile-time constants at examples/bfv.rs:27-30. */
typedef struct { uint64_t n; uint64_t q; uint64_t t; uint64_t b; } zkfhe_bfv_params;
/* configs/<name>.json "params" + "break_points" (README.md:38).  With n_break_* == 0 and replay == 0 the
 * break points are computed (keygen stage); with replay != 0 they are replayed (prover stage). */
typedef struct {
  uint32_t k, n_gate0, n_gate1, n_lookup, n_rlc, unusable_rows, lookup_bits;
  const uint32_t *bp_gate0; uint32_t n_bp_gate0;
  const uint32_t *bp_gate1; uint32_t n_bp_gate1;
  const uint32_t *bp_rlc;   uint32_t n_bp_rlc;
  int replay;
  uint32_t transcript;   /* ZKFHE_TRANSCRIPT_*: part of the verifying key (bound into its digest) */
} zkfhe_bfv_config;

typedef struct zkfhe_bfv_tables zkfhe_bfv_tables;
/* Host-only (no GPU): runs the circuit (examples/bfv.rs:63-304) on the JSON input text (CircuitInput,
 * examples/bfv.rs:50-61) with RLC challenge `gamma` (32-byte LE canonical Fr) and places the cell streams
 * into columns.  keygen_mode != 0 also produces the fixed columns and the copy constraints. */
int zkfhe_bfv_build_tables(const char *input_json, const zkfhe_bfv_params *params, const zkfhe_bfv_config *config,
                           const uint8_t gamma[32], int keygen_mode, zkfhe_bfv_tables **out, char *err, size_t err_len);
void zkfhe_bfv_tables_free(zkfhe_bfv_tables *t);
/* Column counts the circuit needs at 2^k rows (halo2-base auto-configuration, the first half of the reference's keygen):
 * counts_out = { n_gate0, n_gate1, n_lookup, n_rlc }.  Host only. */
int zkfhe_bfv_auto_config(const char *input_json, const zkfhe_bfv_params *params, uint32_t k, uint32_t unusable_rows, uint32_t lookup_bits,
                          uint32_t counts_out[4], char *err, size_t err_len);
/* what: 0 n_advice, 1 n_fixed, 2 n rows, 3 n_instance, 4 n_copies, 5/6/7 number of break points gate0/gate1/rlc,
 *       8/9/10 cells in the phase-0 / phase-1 gate / RLC stream, 11 lookup cells */
size_t zkfhe_bfv_tables_count(const zkfhe_bfv_tables *t, int what);
/* canonical (non-Montgomery) 4 x u64 values */
int zkfhe_bfv_tables_copy_advice(const zkfhe_bfv_tables *t, uint64_t *out);     /* n_advice * n * 4 */
int zkfhe_bfv_tables_copy_fixed(const zkfhe_bfv_tables *t, uint64_t *out);      /* n_fixed * n * 4  */
int zkfhe_bfv_tables_copy_instance(const zkfhe_bfv_tables *t, uint64_t *out);   /* n_instance * 4   */
int zkfhe_bfv_tables_copy_copies(const zkfhe_bfv_tables *t, uint64_t *out);     /* n_copies * 2 (cell = perm_col * n + row) */
int zkfhe_bfv_tables_copy_break_points(const zkfhe_bfv_tables *t, int which, uint32_t *out);

/* Process-wide admission gate of the proofs in flight: at most n of them inside the GPU-heavy middle of a proof (grand products,
 * their commitment, coset extension, quotient) at a time, first come first served; 0 = no gate (default, or ZKFHE_GATE), n < 0 =
 * query.  Returns the previous setting.  Spreads proofs that would otherwise move through the Fiat-Shamir rounds in lockstep; pays
 * when the streams are kept full, not for a batch that starts and ends together.  Ignored by sharded proofs.
 * A limit above 0 also tells the library that the caller keeps the chip full: a proof reads the gate once, at its entry, and with a
 * limit above 0 runs the throughput profile to its end -- it leaves out what only shortens the latency of a lone proof (32 elements
 * per field inversion in the long batch inversions, chunks of 256 points in the table sums of a few columns, no early phase-1
 * commitment where the Poseidon hash is its only reason).  Same proof bytes under either profile.  ZKFHE_PROFILE=latency|throughput
 * overrides the gate's choice; ZKFHE_EARLY_P1 and ZKFHE_BI_CHUNK still win over the profile. */
int zkfhe_prover_gate(int n);

/* `mock` (README.md:18-22, halo2 MockProver::run(..).assert_satisfied()): evaluates every constraint on every row of
 * tables built with keygen_mode != 0 and the same gamma -- gate and RLC-gate identities under their selectors, lookup
 * membership, and both cells of every copy constraint.  *n_failures = number of violated rows / constraints, err = the
 * first one.  Host only.  zkfhe_bfv_tables_poke_advice overwrites one advice cell (negative tests of the checker). */
int zkfhe_bfv_mock_check(const zkfhe_bfv_tables *t, const uint8_t gamma_le[32], uint64_t *n_failures, char *err, size_t err_len);
int zkfhe_bfv_tables_poke_advice(zkfhe_bfv_tables *t, uint32_t column, uint32_t row, const uint8_t value_le[32]);

/* Unsafe seeded test SRS (the reference's gen_srs is an unsafe seeded setup as well, README.md:34): s derived
 * from the seed, g[i] = s^i G, g_lagrange[i] = L_i(s) G, both computed on the GPU and kept as MSM bases. */
typedef struct zkfhe_srs zkfhe_srs;
/* Passing exactly this string as the seed derives s the way the REFERENCE's setup does: halo2-scaffold gen_srs ->
 * ParamsKZG::<Bn256>::setup(k, ChaCha20Rng::from_seed([0u8; 32])), s = Fr::from_u512 of the first 64 bytes of the ChaCha20
 * keystream of the all-zero key (the published RFC 7539 zero-key vector).  Any other seed: Blake2b-512("zkfhe-srs", seed) mod r. */
#define ZKFHE_SRS_HALO2_UNSAFE "halo2:ParamsKZG::setup(k, ChaCha20Rng::from_seed([0u8; 32]))"
int zkfhe_srs_create(zkfhe_ctx *ctx, uint32_t k, const uint8_t *seed, size_t seed_len, zkfhe_srs **out);
/* params/kzg_bn254_<k>.srs (README.md:34; .gitignore:17), the file halo2 `ParamsKZG::write` / `::read` exchange
 * (SerdeFormat::RawBytes): u32 k little-endian | g[2^k] | g_lagrange[2^k] | g2 | s_g2 -- G1 points as x | y, G2 points as
 * x.c0 | x.c1 | y.c0 | y.c1, every coordinate four little-endian u64 Montgomery limbs, i.e. the library's in-memory layout.
 * save: an unsharded SRS made by zkfhe_srs_create, zkfhe_srs_load, or zkfhe_srs_from_points + zkfhe_srs_set_g2.
 * load: checks the frame, that every coordinate is reduced and every point on its curve (as halo2's RawBytes read does). */
int zkfhe_srs_save(zkfhe_ctx *ctx, const zkfhe_srs *srs, const char *path);
/* Releases the host copies of the points an unsharded SRS keeps for zkfhe_srs_save (128 B x 2^k); a later save is refused. */
int zkfhe_srs_drop_host_copy(zkfhe_srs *srs);
int zkfhe_srs_load(zkfhe_ctx *ctx, const char *path, zkfhe_srs **out);
/* The verifier's half, as zkfhe_bfv_verify_g2 takes it: canonical little-endian x.c0 | x.c1 | y.c0 | y.c1 of G2 and s G2.
 * zkfhe_srs_g2: of an SRS in memory (ZKFHE_EINVAL when it has none: from_points without set_g2); zkfhe_srs_file_g2: read from
 * the tail of a params file on the host alone (no GPU: `verify` needs nothing else of the SRS); *k_out = the file's k. */
int zkfhe_srs_g2(const zkfhe_srs *srs, uint8_t g2_le[128], uint8_t s_g2_le[128]);
int zkfhe_srs_set_g2(zkfhe_srs *srs, const uint8_t g2_le[128], const uint8_t s_g2_le[128]);
int zkfhe_srs_file_g2(const char *path, uint32_t *k_out, uint8_t g2_le[128], uint8_t s_g2_le[128]);
/* One ChaCha20 block (RFC 7539 section 2.3; words 12..15 of the state as given): host-only hook that pins the keystream the
 * reference derivation above reads to the published vectors. */
int zkfhe_chacha20_block(const uint8_t key[32], const uint32_t counter_nonce[4], uint8_t out[64]);
/* An SRS from outside (a ceremony file such as the reference's params/kzg_bn254_<k>.srs, README.md:34-38, read by the
 * caller): 2^k points g[i] = s^i G and g_lagrange[i] = L_i(s) G, host memory, affine, Montgomery limbs (halo2curves'
 * in-memory G1Affine).  The library only builds its MSM tables from them; nothing is checked about the ceremony here:
 * zkfhe_srs_check (below) checks the structure of an SRS that has its G2 half, and zkfhe_srs_from_monomial /
 * zkfhe_srs_load_downsized compute g_lagrange themselves for a caller who holds the monomial powers only. */
int zkfhe_srs_from_points(zkfhe_ctx *ctx, uint32_t k, const zkfhe_g1_affine *g_host, const zkfhe_g1_affine *g_lagrange_host, zkfhe_srs **out);
/* An SRS from a ceremony's monomial powers alone: g[i] = s^i G for i < n_g, n_g >= 2^k (a longer list is cut: halo2's
 * ParamsKZG::downsize).  g_lagrange is computed here (zkfhe_g1_fft, inverse).  g2_le / s_g2_le as zkfhe_srs_set_g2, or both NULL.
 * Unsharded.  ZKFHE_EINVAL, message prefixed "srs_from_monomial:", for a NULL argument or exactly one G2 argument, k outside
 * 3..20, n_g < 2^k, a coordinate >= p, a point off its curve, or the identity among the 2^k powers. */
int zkfhe_srs_from_monomial(zkfhe_ctx *ctx, uint32_t k, const zkfhe_g1_affine *g_host, size_t n_g,
                            const uint8_t g2_le[128], const uint8_t s_g2_le[128], zkfhe_srs **out);
/* The same from a halo2 RawBytes params file of k_file >= k: reads the header, the first 2^k points of g and the G2 tail, never the
 * file's g_lagrange.  Refusals as above, prefixed "srs_load_downsized:", and for k_file < k or a short or misframed file. */
int zkfhe_srs_load_downsized(zkfhe_ctx *ctx, const char *path, uint32_t k, zkfhe_srs **out);
/* Checks that an unsharded SRS with its G2 half (g2, s_g2) has the structure of one; *failed = 0 means every check passed.
 *  - powers: with scalars r_i drawn from the seed, A = sum r_i g[i] and B = sum r_i g[i+1] (i < 2^k - 1; one MSM call of two
 *    columns) must satisfy e(A, s_g2) e(-B, g2) = 1 (host pairing): g[i+1] = s g[i] for the s of (g2, s_g2), up to 2^-250.
 *  - Lagrange: for a coefficient column c drawn from the seed, MSM(g, c) = MSM(g_lagrange, NTT(c)): a g_lagrange that is not the
 *    Lagrange form of g passes with probability 1/r.
 *  - generator: g[0] = (1, 2) and both G2 points on the twist curve.
 * seed: 32 bytes the SRS's maker could not predict (NULL: the OS's entropy); a maker who knows the seed can pass a bad SRS.
 * What this does NOT check: that anyone forgot s -- no computation on the points can; and that g2 / s_g2 lie in the prime-order
 * subgroup of the twist: only the curve equation is tested, as halo2's RawBytes read does.
 * ZKFHE_EINVAL with a message for an SRS without G2 (zkfhe_srs_set_g2) and for a sharded SRS. */
#define ZKFHE_SRS_BAD_POWERS 1     /* g is not (g[0], s g[0], s^2 g[0], ...) for the s of (g2, s_g2) */
#define ZKFHE_SRS_BAD_LAGRANGE 2   /* g_lagrange is not the Lagrange form of g */
#define ZKFHE_SRS_BAD_GENERATOR 4  /* g[0] is not the generator (1, 2), or g2 / s_g2 is not on the twist curve */
int zkfhe_srs_check(zkfhe_ctx *ctx, const zkfhe_srs *srs, const uint8_t seed[32], uint32_t *failed);
/* The same seeded setup, but only this rank's point range of both halves (1 / world of the table memory); keygen and prove
 * called with it shard every commitment over `comm` (see "intra-proof multi-GPU").  comm must outlive the SRS. */
int zkfhe_srs_create_sharded(zkfhe_ctx *ctx, zkfhe_comm *comm, uint32_t k, const uint8_t *seed, size_t seed_len, zkfhe_srs **out);
int zkfhe_srs_destroy(zkfhe_ctx *ctx, zkfhe_srs *srs);
/* zkfhe_basis_table_bits of the Lagrange half of the SRS (the basis of the advice / permutation / lookup commitments). */
int zkfhe_srs_table_bits(const zkfhe_srs *srs, int *wide_calls);
/* bits[0] / bits[1]: digit width of the monomial / Lagrange half's table (0 = none); *bytes: resident bytes of both; *narrowed: a
 * half is narrower than its budget allowed (no room on the device at creation: slower calls, same results).  Outputs optional. */
int zkfhe_srs_table_info(const zkfhe_srs *srs, int bits[2], uint64_t *bytes, int *narrowed);

/* keygen (README.md:28-38): circuit structure from the (empty) input, fixed + sigma polynomials, their
 * commitments, the vk digest; everything the prover needs stays resident in HBM. */
typedef struct zkfhe_bfv_pk zkfhe_bfv_pk;
int zkfhe_bfv_keygen(zkfhe_ctx *ctx, const zkfhe_srs *srs, const char *input_json, const zkfhe_bfv_params *params,
                     const zkfhe_bfv_config *config, zkfhe_bfv_pk **out);
int zkfhe_bfv_pk_destroy(zkfhe_ctx *ctx, zkfhe_bfv_pk *pk);
/* A key keeps one prover workspace per context that proved against it (0.3 GB at k = 13, several GB at k = 19) until the
 * key is destroyed.  Call this before zkfhe_ctx_destroy when the key outlives the context. */
int zkfhe_bfv_pk_release_ctx(zkfhe_ctx *ctx, zkfhe_bfv_pk *pk);
/* 32-byte LE vk digest; counts of fixed / sigma commitments; the commitments as canonical affine (x||y, 64 B each) */
int zkfhe_bfv_pk_info(const zkfhe_bfv_pk *pk, uint8_t vk_digest[32], uint32_t *n_fixed, uint32_t *n_sigma);
int zkfhe_bfv_pk_commitments(const zkfhe_bfv_pk *pk, uint8_t *fixed_out, uint8_t *sigma_out);
/* Per-public-key transcript cache.  The instance column starts with pk0 | pk1 (reference examples/bfv.rs:118-119), the same
 * 2 N values for every encryption under one BFV public key; the prover keeps the Fiat-Shamir state after `vk digest | pk0 | pk1`
 * for the last few public keys it has seen with this proving key and starts a proof whose pk0 | pk1 match from there (k = 13:
 * 1 024 of the 2 561 sequential Poseidon permutations before the first challenge).  Same state, same bytes.  Nothing beyond the
 * public key is cached.  capacity >= 0 sets how many keys are remembered (default 8, ZKFHE_PREFIX_CACHE; 0 = off; at most 64),
 * negative only queries; hits / misses / entries are optional outputs. */
int zkfhe_bfv_pk_prefix_cache(const zkfhe_bfv_pk *pk, int capacity, uint64_t *hits, uint64_t *misses, uint64_t *entries);
/* Announce a proof ahead of time.  The first challenge of a proof stands behind one SEQUENTIAL sponge over the 5 N + 1 public inputs
 * (reference examples/bfv.rs:118-122; with the reference's Poseidon transcript 10 241 permutations at N = 4096, 40 961 at N = 16384:
 * 30 / 120 ms on a core, as long as the proof's GPU work) that depends on the input alone.  A caller that knows the input of a LATER
 * proof calls this while the current proof is on the GPU: the public inputs are parsed and absorbed on a helper thread, and the
 * zkfhe_bfv_prove of the same input_json (the same bytes) starts from the parked state (it waits for it if it is not complete yet).
 * The call returns after copying the text.  One-shot: an announcement serves one proof, the oldest announcement of a text first; at
 * most 16 may be pending (ZKFHE_EINVAL beyond).  An input that does not parse serves nobody (zkfhe_bfv_prove words the error).  Same
 * state, same proof bytes.  Host only.  started / taken / pending: optional counters; input_json == NULL only reads them. */
int zkfhe_bfv_pk_prehash(const zkfhe_bfv_pk *pk, const char *input_json, uint64_t *started, uint64_t *taken, uint64_t *pending);
int zkfhe_bfv_pk_break_points(const zkfhe_bfv_pk *pk, int which, uint32_t *out, uint32_t *count);

/* Serialised verifying key: magic "ZKFHEVK2", 8 x u32 configuration (k, n_gate0, n_gate1, n_lookup, n_rlc, unusable_rows,
 * lookup_bits, transcript), u32 n_fixed, u32 n_sigma, 32-byte vk digest, then the fixed and sigma commitments as canonical
 * affine x||y (64 B each).  What `keygen` writes to data/<name>.vk. */
int zkfhe_bfv_pk_export_vk(const zkfhe_bfv_pk *pk, uint8_t *out, size_t cap, size_t *len);
/* Parity hook for the GPU witness generator: the phase-1 gate-context cell stream of examples/bfv.rs:171-301 (1 231 992 cells at
 * the reference's parameters) as produced on the device, canonical 32-byte little-endian values, for a caller-chosen challenge
 * gamma.  cells_out == NULL only returns the cell count. */
int zkfhe_bfv_witness_stream(zkfhe_ctx *ctx, const zkfhe_bfv_pk *pk, const char *input_json, const uint8_t gamma_le[32], uint8_t *cells_out,
                             size_t cap_cells, size_t *n_cells);
/* Lookup argument, step 1 (halo2 lookup::prover `permute_expression_pair`) for the 8-bit table
 * {0..255} over `usable_rows` rows: column c (Montgomery Fr, n rows) -> A' = the inputs sorted, S' = the table permuted so
 * that S'[i] = A'[i] wherever A'[i] differs from A'[i-1], the unused table values filling the other rows in ascending
 * order.  Rows >= usable_rows of the outputs are left untouched (the prover blinds them).  *not_in_table = 1 if an input
 * exceeds 255.  One workgroup per column. */
int zkfhe_lookup_permute(zkfhe_ctx *ctx, const zkfhe_fr *cols_dev, size_t n_cols, size_t n, uint32_t usable_rows, zkfhe_fr *a_dev,
                         zkfhe_fr *s_dev, int *not_in_table);
/* Proving key on disk (the reference's keygen writes data/<name>.pk, README.md:38): configuration, break points, commitments
 * and the fixed / permutation columns; the extended-domain tables are rebuilt on load.  A key is bound to the SRS it was
 * generated with. */
int zkfhe_bfv_pk_save(zkfhe_ctx *ctx, const zkfhe_bfv_pk *pk, const char *path);
int zkfhe_bfv_pk_load(zkfhe_ctx *ctx, const zkfhe_srs *srs, const char *path, zkfhe_bfv_pk **out);

/* data/<name>.snark (README.md:42-52).  snark-verifier-sdk's `Snark { protocol, instances: Vec<Vec<Fr>>, proof: Vec<u8> }` is
 * written with bincode (fixed-width little-endian integers, u64 lengths); its `protocol` field is the compiled PlonkProtocol of
 * the reference's constraint system, which this library does not have.  This container keeps the two
 * fields that ARE common, byte for byte as bincode writes them, behind a 16-byte header:
 *   "ZKFHESN2" | u64 protocol_len = 0 (absent) | u64 1 | u64 n | n x Fr | u64 proof_len | proof bytes
 * with Fr as halo2curves' serde derives it: four little-endian u64 limbs of the MONTGOMERY form (x * 2^256 mod r) -- so a Rust
 * reader skips 16 bytes and `bincode::deserialize::<(Vec<Vec<Fr>>, Vec<u8>)>`s the rest.  Host only.
 * encode: instances as canonical 32-byte LE scalars; out = NULL / cap too small: *len = bytes needed (ZKFHE_EINVAL if cap > 0).
 * decode: also accepts the round-1..3 container ("ZKFHESN1" | u64 n | n canonical scalars | proof); NULL outputs = sizes only. */
int zkfhe_snark_encode(const uint8_t *instances_le, size_t n_instances, const uint8_t *proof, size_t proof_len, uint8_t *out, size_t cap, size_t *len);
int zkfhe_snark_decode(const uint8_t *snark, size_t snark_len, uint8_t *instances_le, size_t *n_instances, uint8_t *proof, size_t *proof_len);

/* verify (README.md:48-52), host CPU only (no GPU, like the reference's verifier): replays the transcript, checks the
 * quotient identity at x, and ends in one BN254 pairing-product check.  instances: n_instances canonical 32-byte LE
 * scalars.  srs_seed: the seed the (unsafe, test) SRS was derived from.  *accepted = 1 iff the proof verifies; a
 * malformed proof is reported as accepted = 0 with the reason in err. */
int zkfhe_bfv_verify(const uint8_t *vk_bytes, size_t vk_len, const uint8_t *instances, size_t n_instances, const uint8_t *proof,
                     size_t proof_len, const uint8_t *srs_seed, size_t seed_len, int *accepted, char *err, size_t err_len);
/* The same check against the verifier's half of an external SRS: G2 and s*G2 as four 32-byte little-endian canonical Fq values
 * each (x.c0, x.c1, y.c0, y.c1), the layout of halo2curves' G2Affine coordinates. */
int zkfhe_bfv_verify_g2(const uint8_t *vk_bytes, size_t vk_len, const uint8_t *instances, size_t n_instances, const uint8_t *proof, size_t proof_len,
                        const uint8_t g2[128], const uint8_t s_g2[128], int *accepted, char *err, size_t err_len);

/* Batch verification (halo2 KZG AccumulatorStrategy / verify_proof over many snarks): n_proofs proofs under ONE verifying key,
 * proof j with n_instances[j] canonical scalars at instances[j] and proof_lens[j] bytes at proofs[j].  accepted[j] and the
 * reason written to errs + j * err_stride (err_stride bytes each; errs may be NULL) are exactly what zkfhe_bfv_verify (srs_seed,
 * when g2 == NULL) or zkfhe_bfv_verify_g2 (g2 and s_g2 both given) answers for that proof.  Host memory only; the context's GPU
 * decompresses every proof point (zkfhe_g1_decompress) and computes each proof's SHPLONK combination F_j (zkfhe_msm_segmented);
 * the transcripts are replayed on host threads (the usable CPUs: affinity mask, OMP_NUM_THREADS), proofs of one BFV public key
 * (the same pk0 | pk1, the first 2 N of 5 N + 1 instances) from one shared transcript state.  Then ONE pairing check:
 *     e(sum_j r_j F_j, G2) e(-sum_j r_j W_j, s G2) = 1      (W_j = the proof's h2)
 * over the proofs that got that far; if it fails, every one of them is checked on its own from its F_j and W_j.
 * Randomisers: r_j = the low 128 bits of Blake2b-512(personalisation "zkfhe-batch-r"; vk digest | D | j as u64 LE), 1 if zero,
 * with D = Blake2b-512("zkfhe-batch-D"; for every proof in order: u64 n_instances | instances | u64 proof_len | proof): fixed by
 * the whole batch, so no prover can choose a proof that cancels against another's defect.  Proofs go to the GPU in chunks of
 * 256.  Returns ZKFHE_EINVAL for n_proofs = 0 or NULL arguments; a malformed proof or vk is a rejection, not an error. */
int zkfhe_bfv_verify_batch(zkfhe_ctx *ctx, const uint8_t *vk_bytes, size_t vk_len, size_t n_proofs, const uint8_t *const *instances,
                           const size_t *n_instances, const uint8_t *const *proofs, const size_t *proof_lens, const uint8_t *srs_seed,
                           size_t seed_len, const uint8_t *g2, const uint8_t *s_g2, int *accepted, char *errs, size_t err_stride);

/* prove (README.md:42-44): witness generation + create_proof.
 * seed: 32 bytes; every blinding scalar of the proof is derived from it (Blake2b(seed || counter)).  ZERO KNOWLEDGE RESTS
 * ON THE SEED: it must be fresh, secret randomness for every proof (the reference draws StdRng::from_entropy()); a known
 * or reused seed makes the blinding rows predictable and the openings then leak the witness (u, e0, e1, m).  A fixed
 * seed is only for reproducible tests.
 * proof_out must hold proof_cap bytes; *proof_len receives the length.  instances_out (may be NULL): canonical
 * 32-byte LE scalars; *n_instances is its capacity on entry and the instance count on return -- if the capacity is too
 * small the call fails with ZKFHE_EINVAL and *n_instances holds the required count.
 * timings_ms (may be NULL): [witness, commit, quotient, open, total]. */
int zkfhe_bfv_prove(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_bfv_pk *pk, const char *input_json,
                    const uint8_t seed[32], uint8_t *proof_out, size_t proof_cap, size_t *proof_len,
                    uint8_t *instances_out, size_t *n_instances, float *timings_ms);

/* prove from machine words: the input of zkfhe_bfv_prove as N uint64_t per polynomial (the key's N), in CircuitInput order
 * (highest degree first), residues as the JSON would spell them; cyclo is x^N + 1.  For the same seed the proof bytes and
 * instances equal those of zkfhe_bfv_prove on the JSON that spells the same numbers, and exactly the inputs it refuses are refused
 * (words outside the machine-word path are rendered as that JSON and take the text path).  The per-key prefix cache applies
 * (it is keyed on values); announcements of zkfhe_bfv_pk_prehash are keyed on text and serve zkfhe_bfv_prove alone.  The seed
 * carries the same warning as zkfhe_bfv_prove's. */
typedef struct {
  const uint64_t *pk0, *pk1, *m, *u, *e0, *e1, *c0, *c1;
} zkfhe_bfv_words;
int zkfhe_bfv_prove_words(zkfhe_ctx *ctx, const zkfhe_srs *srs, const zkfhe_bfv_pk *pk, const zkfhe_bfv_words *in, const uint8_t seed[32],
                          uint8_t *proof_out, size_t proof_cap, size_t *proof_len, uint8_t *instances_out, size_t *n_instances, float *timings_ms);

/* ---- BFV key generation / encryption / decryption on the GPU (what zkfhe_bfv_prove proves: the ciphertext and u, e0, e1) ----
 * Polynomials: N uint64_t each, CircuitInput order (highest degree first), every coefficient a residue in [0, Q) (-1 is Q - 1):
 * the output of zkfhe_bfv_encrypt goes to zkfhe_bfv_prove_words as it is.  Parameters: zkfhe_bfv_params with N a power of two,
 * 8 <= N <= 32768, 2 <= Q < 2^63, 2 <= T < Q, 1 <= B < min(Q, 1024); delta = floor(Q / T).  Anything else is ZKFHE_EINVAL.
 * Randomness: ChaCha20 keyed by the 32-byte seed, state words 12..15 = {block, domain, index_lo, index_hi} (the layout of
 * zkfhe_chacha20_block); word w of a stream is its w-th little-endian u64 and array position p reads word p.  Domains:
 * encryption 1 = u, 2 = e0, 3 = e1 with index = first_index + j for message j; key generation 4 = s, 5 = a, 6 = e with index 0.
 * Samplers (branch-free, no secret-dependent address): ternary ((w * 3) >> 64) - 1; uniform (x * Q) >> 128 with
 * x = w[2p] + 2^64 w[2p + 1]; error -B + #{i : w >= T_i} over the 2 B thresholds of zkfhe_bfv_error_cdt.
 * ENCRYPTION SEEDS ARE SECRET AND FRESH, like the seed of zkfhe_bfv_prove: whoever knows the seed knows u, e0, e1 and with
 * them m.  Reusing a (seed, index) pair reuses u, and two ciphertexts that share u reveal the difference of their messages.
 * A fixed seed is only for reproducible tests. */
/* a * s mod (x^N + 1, Q) on device pointers, exact: a_count (1 = one a shared by all, or n_polys) polynomials a of integers
 * below 2^64, n_polys ternary polynomials s with coefficients in {0, 1, Q - 1} (otherwise *not_ternary = 1 and ZKFHE_EINVAL, out
 * undefined); out: n_polys polynomials.  Three-prime RNS negacyclic NTT in LDS, CRT epilogue (bfv_enc.hip).  Waits. */
int zkfhe_poly_mul_ternary_negacyclic(zkfhe_ctx *ctx, const uint64_t *a_dev, size_t a_count, const uint64_t *s_dev, size_t n_polys,
                                      uint64_t n, uint64_t q, uint64_t *out_dev, int *not_ternary);
/* Host only: the 2 B thresholds T_i = round(2^64 P(X <= -B + i)) of the discrete Gaussian (sigma 3.2) restricted to [-B, B] and
 * renormalised; *count = 2 B, thresholds may be NULL.  This table defines the error sampler. */
int zkfhe_bfv_error_cdt(const zkfhe_bfv_params *params, uint64_t *thresholds, size_t *count);
/* sk = s, pk0 = -(a s + e), pk1 = a (zk-fhe_amd/inputs.py keygen); host arrays of N. */
int zkfhe_bfv_fhe_keypair(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint8_t seed[32], uint64_t *sk_out, uint64_t *pk0_out,
                          uint64_t *pk1_out);
/* n_msgs encryptions under one public key: c0 = pk0 u + delta m + e0, c1 = pk1 u + e1 in Z_Q[x]/(x^N + 1); host arrays of
 * n_msgs x N.  pk0, pk1 below Q and every m coefficient in [0, T/2] or [Q - T/2, Q - 1] (the circuit's range check), else
 * ZKFHE_EINVAL.  pk0 and pk1 are transformed once per call. */
int zkfhe_bfv_encrypt(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *pk0, const uint64_t *pk1, size_t n_msgs,
                      const uint64_t *m, const uint8_t seed[32], uint64_t first_index, uint64_t *u_out, uint64_t *e0_out,
                      uint64_t *e1_out, uint64_t *c0_out, uint64_t *c1_out);
/* m = round(T [c0 + c1 s]_Q / Q) centred mod T, as a residue mod Q (inputs.py decrypt); host arrays of n_msgs x N. */
int zkfhe_bfv_decrypt(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, size_t n_msgs, const uint64_t *c0,
                      const uint64_t *c1, uint64_t *m_out);
/* zkfhe_prof_read slots of the BFV encryption kernels (algorithmic bytes: words read and written) */
#define ZKFHE_PROF_BFV_SAMPLE 5     /* k_bfv_sample */
#define ZKFHE_PROF_RNS_NTT 6        /* k_rns_ntt */
#define ZKFHE_PROF_RNS_EPILOGUE 7   /* k_rns_epilogue (every three-prime product of the BFV calls) */

/* ---- BFV evaluation on the GPU: computing on verified ciphertexts (bfv_eval.hip) ----
 * The conventions above: host arrays, N uint64_t per polynomial in CircuitInput order, residues in [0, Q), batches n x N, the
 * parameter checks of zkfhe_bfv_encrypt.  Plaintexts m are in [0, T/2] or [Q - T/2, Q - 1].  Every call refuses, with ZKFHE_EINVAL and
 * a message: a ciphertext or key coefficient >= Q, a plaintext out of range, a non-ternary sk, base_bits outside [1, 32], an m_count
 * other than 1 or n.  The output of an evaluation is NOT a fresh encryption: zkfhe_bfv_prove_words cannot prove it, and its noise
 * grows with every operation (zkfhe_bfv_noise).  Every call waits for its result. */
/* n pairwise a + b (subtract = 0) or a - b (subtract != 0) mod Q */
int zkfhe_bfv_add(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0,
                  const uint64_t *b1, int subtract, uint64_t *out0, uint64_t *out1);
/* one ciphertext (out0, out1 of N), the sum of all n_cts mod Q: the tally.  Uploaded in chunks. */
int zkfhe_bfv_sum(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_cts, const uint64_t *c0, const uint64_t *c1, uint64_t *out0,
                  uint64_t *out1);
/* out0 = c0 + floor(Q/T) m mod Q, out1 = c1; m_count = 1 (one plaintext for every ciphertext) or n */
int zkfhe_bfv_add_plain(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1, size_t m_count,
                        const uint64_t *m, uint64_t *out0, uint64_t *out1);
/* (c0 m, c1 m) mod (x^N + 1, Q); m_count = 1 or n */
int zkfhe_bfv_mul_plain(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1, size_t m_count,
                        const uint64_t *m, uint64_t *out0, uint64_t *out1);
/* Host only: *l = ceil(bitlen(Q - 1) / w), the number of relinearization digits of width w = base_bits in [1, 32] */
int zkfhe_bfv_relin_digits(const zkfhe_bfv_params *params, int base_bits, size_t *l);
/* the relinearization key of sk: l pairs (rlk0, rlk1 of l x N), rlk0_i = -(a_i s + e_i) + 2^(i w) s^2 mod Q, rlk1_i = a_i, with a_i
 * uniform from ChaCha20 domain 7 and e_i an error sample from domain 8, both with index i (the samplers of zkfhe_bfv_encrypt).  The
 * key is public; its SEED IS SECRET like any key seed (it gives a_i and e_i, and with them s^2). */
int zkfhe_bfv_relin_keygen(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, const uint8_t seed[32], int base_bits,
                           uint64_t *rlk0, uint64_t *rlk1);
/* n ciphertext products, relinearized, defined exactly: every input coefficient lifted to its centred integer (v - Q if
 * v > floor(Q/2)); x0 = a0 b0, x1 = a0 b1 + a1 b0, x2 = a1 b1 exactly over Z in Z[x]/(x^N + 1); c^_j = floor((2 T x_j + Q) / 2Q)
 * mod Q; digits d_i = (c^2 >> i w) & (2^w - 1) of c^2 in [0, Q); out0 = c^0 + sum_i d_i rlk0_i, out1 = c^1 + sum_i d_i rlk1_i mod Q.
 * rlk0, rlk1: l x N from zkfhe_bfv_relin_keygen with the same base_bits; they are transformed once per call. */
int zkfhe_bfv_mul(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *a0, const uint64_t *a1, const uint64_t *b0,
                  const uint64_t *b1, const uint64_t *rlk0, const uint64_t *rlk1, int base_bits, uint64_t *out0, uint64_t *out1);
/* per ciphertext, max over coefficients of |[c0 + c1 s - floor(Q/T) m]_Q| (centred), m its decryption (zkfhe_bfv_decrypt): the
 * noise that decryption tolerates while it stays below floor(Q/T) / 2 */
int zkfhe_bfv_noise(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, size_t n, const uint64_t *c0, const uint64_t *c1,
                    uint64_t *noise_out);
/* Host only. The largest n_terms the two calls below accept, saturating at SIZE_MAX.
 * P = 3291839576991896151990342918866792881986076673 is the product of the five RNS primes.
 *   plain == 0: the largest n with n * 2 N floor(Q/2)^2          <= floor(P/2)
 *   plain != 0: the largest n with n *   N floor(Q/2) floor(T/2) <= floor(P/2) */
int zkfhe_bfv_dot_max_terms(const zkfhe_bfv_params *params, int plain, size_t *max_terms);
/* n_groups inner products of n_terms relinearized products each (bfv_dot.hip): one rescale and one relinearization per sum.
 * a0, a1: [n_groups][n_terms][N].
 * b0, b1: [b_groups][n_terms][N], b_groups = 1 (one b vector for every group) or n_groups.
 * Defined exactly. Every coefficient is lifted to its centred integer.
 *   x0 = sum_i a0_i b0_i, x1 = sum_i (a0_i b1_i + a1_i b0_i), x2 = sum_i a1_i b1_i,
 *   over Z in Z[x]/(x^N + 1).
 *   c^_j = floor((2 T x_j + Q) / 2Q) mod Q.
 * Then the digits and key sum of zkfhe_bfv_mul:
 *   out0 = c^0 + sum_i d_i rlk0_i, out1 = c^1 + sum_i d_i rlk1_i.
 * out0, out1: [n_groups][N].
 * n_terms = 1 is zkfhe_bfv_mul bit for bit.
 * For n_terms > 1 the result differs from the sum of the products only in the roundings.
 * Refused with ZKFHE_EINVAL and a message "bfv_dot: ...", in this order and before any pass over the inputs and any device work: a
 * NULL argument, a zero count or bad parameters; base_bits outside [1, 32]; b_groups other than 1 or n_groups; n_terms above
 * zkfhe_bfv_dot_max_terms (the message states the limit).  Then the range checks of zkfhe_bfv_mul.  The noise of the result grows
 * with n_terms (zkfhe_bfv_noise). */
int zkfhe_bfv_dot(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_groups, size_t n_terms,
                  const uint64_t *a0, const uint64_t *a1, size_t b_groups,
                  const uint64_t *b0, const uint64_t *b1,
                  const uint64_t *rlk0, const uint64_t *rlk1, int base_bits,
                  uint64_t *out0, uint64_t *out1);
/* n_groups weighted sums with public weights:
 *   out_j = sum_i c_j,i m_i mod (x^N + 1, Q), j = 0, 1.
 * This is bit for bit the zkfhe_bfv_sum of the zkfhe_bfv_mul_plain products.
 * c0, c1: [n_groups][n_terms][N].
 * m: [m_groups][n_terms][N], m_groups = 1 or n_groups, plaintexts in the range of zkfhe_bfv_mul_plain.
 * Refusals as for zkfhe_bfv_dot, with the prefix "bfv_dot_plain:" and the limit of plain != 0. */
int zkfhe_bfv_dot_plain(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_groups, size_t n_terms,
                        const uint64_t *c0, const uint64_t *c1, size_t m_groups, const uint64_t *m,
                        uint64_t *out0, uint64_t *out1);
/* zkfhe_prof_read slots of the BFV evaluation kernels */
#define ZKFHE_PROF_BFV_TENSOR 8            /* k_bfv_tensor */
#define ZKFHE_PROF_BFV_RELIN 9             /* k_key_switch on c^2 itself (the relinearization) */
#define ZKFHE_PROF_BFV_EVAL_EPILOGUE 10    /* k_eval_epilogue */
#define ZKFHE_PROF_BFV_ELEMENTWISE 11      /* k_bfv_sum, k_bfv_add */
#define ZKFHE_PROF_BFV_DOT 20              /* k_bfv_dot_acc, and k_bfv_dot_fold where a pass is split into slices */

/* ---- Threshold BFV on the GPU: collective keys and decryption by shares (bfv_threshold.hip) ----
 * The multiparty BFV of Mouchet et al. (collective key generation, relinearization key generation, threshold decryption with
 * smudging noise), so that voters encrypt to a key the committee holds jointly and only the committee together opens the tally.
 * P parties; party i holds a ternary s_i; the collective secret s = sum_i s_i is never formed by the library.  The conventions
 * above: host arrays, N uint64_t per polynomial in CircuitInput order, residues in [0, Q), the parameter checks of
 * zkfhe_bfv_encrypt; every call waits for its result.  Randomness: the ChaCha20 streams and samplers of zkfhe_bfv_encrypt;
 * domains 1 to 8 keep their meaning and the new ones are 9 to 13:
 *   CRS a of the public key           crs_seed (public)    domain 5, index 0   uniform mod Q
 *   s_i, e_i of a key share           party_seed (secret)  domains 4, 6, index 0   ternary, error
 *   CRS a_j of the relin key, j < l   crs_seed             domain 7, index j   uniform mod Q
 *   smudging noise of share j         share seed (secret)  domain 9, index first_index + j   uniform mod 2E + 1, minus E
 *   u_i (both relin rounds)           party_seed           domain 10, index 0   ternary
 *   e0_ij, e1_ij (round 1), e2_ij     party_seed           domains 11, 12, 13, index j   error
 * Every call refuses, with ZKFHE_EINVAL and a message: a NULL argument, a zero n_parties, n_polys or n_cts, a coefficient >= Q in
 * any input, a non-ternary sk_i, base_bits outside [1, 32], and 2 E + 1 > floor(Q/T).
 * PARTY SEEDS AND SHARE SEEDS ARE SECRET, like every seed here: a party seed gives s_i.  NEVER REUSE a (share seed, index) pair on
 * a different c1: two shares with the same noise give (c1 - c1') s_i.  The same party_seed must be used in both relinearization
 * rounds (u_i is drawn from it twice).  The smudging bound E is the caller's choice: the library claims no statistical hiding for
 * it, and at the k = 13 parameters (29-bit Q, T = 7) there is little room between the noise and floor(Q/T) / 2.
 * zkfhe_bfv_noise refuses the collective s (it is not ternary): a caller who wants the noise computes it from s = sum_i s_i. */
/* party i's key share: sk = s_i, pk0_share = -(a s_i + e_i) mod (x^N + 1, Q), pk1 = a.  With crs_seed == party_seed the output
 * is zkfhe_bfv_fhe_keypair(party_seed) bit for bit.  The collective pk0 = zkfhe_bfv_share_aggregate of the pk0 shares. */
int zkfhe_bfv_keygen_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint8_t crs_seed[32], const uint8_t party_seed[32],
                           uint64_t *sk_out, uint64_t *pk0_share_out, uint64_t *pk1_out);
/* out = sum_i shares[i] mod Q; shares: n_parties x n_polys x N, out: n_polys x N.  It forms the collective pk0 (n_polys = 1), the
 * round-1 h0 | h1 (2 l) and the final rlk0 (l). */
int zkfhe_bfv_share_aggregate(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_polys, const uint64_t *shares,
                              uint64_t *out);
/* relinearization key, round 1 of party i, l = zkfhe_bfv_relin_digits(base_bits) rows each, w = base_bits:
 * h0_i[j] = -u_i a_j + 2^(j w) s_i + e0_ij,  h1_i[j] = s_i a_j + e1_ij  mod (x^N + 1, Q). */
int zkfhe_bfv_relin_share1(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t crs_seed[32],
                           const uint8_t party_seed[32], int base_bits, uint64_t *h0_out, uint64_t *h1_out);
/* round 2 of party i on the round-1 aggregates h0, h1 (l x N each): r_i[j] = s_i h0[j] + (u_i - s_i) h1[j] + e2_ij, u_i drawn again
 * from party_seed.  The collective key is rlk0 = zkfhe_bfv_share_aggregate of the r_i and rlk1 = h1; it satisfies
 * rlk0[j] + rlk1[j] s = 2^(j w) s^2 + s e0_j + u e1_j + e2_j (e0_j, e1_j, e2_j, u the sums over the parties), so zkfhe_bfv_mul
 * takes it unchanged with the same base_bits. */
int zkfhe_bfv_relin_share2(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t party_seed[32], int base_bits,
                           const uint64_t *h0, const uint64_t *h1, uint64_t *r_out);
/* party i's decryption shares of n_cts ciphertexts: d_j = c1_j s_i + e_j mod Q, e_j the smudging noise of stream (seed, 9,
 * first_index + j) with E = smudge_bound (E = 0: no noise); c1, d_out: n_cts x N. */
int zkfhe_bfv_decrypt_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, size_t n_cts, const uint64_t *c1,
                            const uint8_t seed[32], uint64_t first_index, uint64_t smudge_bound, uint64_t *d_out);
/* m = the rounding of zkfhe_bfv_decrypt applied to [c0 + sum_i d_i]_Q; c0, m_out: n_cts x N, d: n_parties x n_cts x N.  With one
 * party and E = 0 this is zkfhe_bfv_decrypt(sk) bit for bit. */
int zkfhe_bfv_decrypt_combine(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_cts, const uint64_t *c0,
                              const uint64_t *d, uint64_t *m_out);
/* zkfhe_prof_read slots of the threshold kernels (algorithmic bytes: words read and written); the CRT epilogue of the share calls
 * (k_rns_epilogue) counts in ZKFHE_PROF_RNS_EPILOGUE */
#define ZKFHE_PROF_BFV_SHARE_SUM 12         /* k_bfv_share_sum */
#define ZKFHE_PROF_BFV_DECRYPT_COMBINE 13   /* k_bfv_decrypt_combine */

/* ---- Collective refresh and key switching (bfv_refresh.hip) ----
 * Two more protocols of Mouchet et al. for a committee that holds s = sum_i s_i jointly.  Collective refresh re-encrypts a worn
 * ciphertext into a nearly noiseless one under the same collective key without anyone seeing the plaintext, so that
 * mul -> refresh -> mul -> ... has no depth limit at a single-word Q.  Public collective key switching (PCKS) re-encrypts a
 * ciphertext from the collective secret to any public key (an auditor, a recipient, a second committee): the committee never sees
 * the plaintext and the recipient need not be online.  The conventions of "Threshold BFV": host arrays, N uint64_t per polynomial
 * in CircuitInput order, residues in [0, Q), the parameter checks of zkfhe_bfv_encrypt; every call waits for its result.  Below,
 * delta = floor(Q/T), P = n_parties, E = smudge_bound, B the error bound of the parameters.
 * Randomness: the ChaCha20 streams and samplers of zkfhe_bfv_encrypt.  Domains 1 to 15 keep their meaning and the new ones are 16
 * to 22; in every row the index is first_index + j for ciphertext j:
 *   PCKS u_ij                 share seed (secret)  domain 16   ternary
 *   PCKS e0_ij                share seed           domain 17   uniform mod 2E + 1, minus E
 *   PCKS e1_ij                share seed           domain 18   error
 *   refresh CRS a_j           crs_seed (public)    domain 19   uniform mod Q
 *   refresh mask M_ij         share seed           domain 20   uniform mod T (the uniform sampler with modulus T)
 *   refresh e0_ij             share seed           domain 21   uniform mod 2E + 1, minus E
 *   refresh e1_ij             share seed           domain 22   error
 * Refusals: all four calls refuse with ZKFHE_EINVAL and a message prefixed "bfv_pcks_share:", "bfv_pcks_combine:",
 * "bfv_refresh_share:" or "bfv_refresh_combine:", in this order and before any work on the ciphertexts: (1) a NULL argument, a zero
 * n_parties or n_cts, or bad parameters; (2) 2 E + 1 > delta (share calls); (3) any input coefficient >= Q; (4) a non-ternary sk_i.
 * No output is written then.
 * SHARE SEEDS ARE SECRET, like every seed here.  NEVER REUSE a (share seed, index) pair: a second refresh share with the same mask
 * and noise on another c1 gives (c1 - c1') s_i, and a second PCKS share with the same u_ij gives the same.  E is the caller's
 * choice; the library claims no statistical hiding for it.  crs_seed and first_index of a refresh are PUBLIC and agreed by all
 * parties (every party and the combiner must pass the same pair), and THEY MUST DIFFER BETWEEN REFRESHES: a_j repeated under two
 * refreshes relates their outputs. */
/* party i's key-switch shares of n_cts ciphertexts towards the public key (pk0_to, pk1_to), mod (x^N + 1, Q):
 *   h0_ij = s_i c1_j + u_ij pk0_to + e0_ij,   h1_ij = u_ij pk1_to + e1_ij.
 * c1, h0_out, h1_out: n_cts x N; pk0_to, pk1_to: N. */
int zkfhe_bfv_pcks_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint64_t *pk0_to,
                         const uint64_t *pk1_to, size_t n_cts, const uint64_t *c1, const uint8_t seed[32], uint64_t first_index,
                         uint64_t smudge_bound, uint64_t *h0_out, uint64_t *h1_out);
/* out0 = c0 + sum_i h0_i, out1 = sum_i h1_i mod Q; c0, out0, out1: n_cts x N, h0, h1: n_parties x n_cts x N.  If pk0_to + pk1_to s'
 * = -e', then out0 + out1 s' = [c0 + c1 s] - u e' + sum e0 + (sum e1) s' (u, e0, e1 summed over the parties): the same plaintext
 * under s', with that much added noise.  The recipient decrypts with zkfhe_bfv_decrypt, or a second committee with its shares. */
int zkfhe_bfv_pcks_combine(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_cts, const uint64_t *c0,
                           const uint64_t *h0, const uint64_t *h1, uint64_t *out0, uint64_t *out1);
/* party i's refresh shares of n_cts ciphertexts, mod (x^N + 1, Q), a_j the CRS stream (crs_seed, 19, first_index + j):
 *   h0_ij = s_i c1_j - delta M_ij + e0_ij,   h1_ij = -s_i a_j + delta M_ij + e1_ij.
 * c1, h0_out, h1_out: n_cts x N. */
int zkfhe_bfv_refresh_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t crs_seed[32],
                            size_t n_cts, const uint64_t *c1, const uint8_t seed[32], uint64_t first_index, uint64_t smudge_bound,
                            uint64_t *h0_out, uint64_t *h1_out);
/* the refreshed ciphertexts, per coefficient:
 *   v = [c0 + sum_i h0_i]_Q;  mu = floor((2 T v + Q) / 2Q) mod T, in [0, T) (the rounding of zkfhe_bfv_decrypt before centring);
 *   out0 = delta mu + sum_i h1_i mod Q;  out1 = a_j, regenerated from crs_seed and first_index.
 * c0, out0, out1: n_cts x N, h0, h1: n_parties x n_cts x N.  mu is the plaintext masked by sum_i M_i mod T: nobody sees the plaintext.
 * Correctness condition (sufficient, not tight): the result decrypts to the input's plaintext under s = sum_i s_i whenever
 *   noise(input) + P E + (P + 1) (Q mod T) < delta / 2 - T.
 * Noise bound: the result's noise is then at most P B + (P + 1) (Q mod T), whatever the input's noise was (checked numerically on
 * the CPU at N = 8 ... 32, 29-, 60- and 62-bit Q, 1 to 5 parties); at the k = 13 parameters with P = 3 that is 61.
 * CRS agreement: first_index and crs_seed are public, the same for all parties and the combiner, and differ between refreshes. */
int zkfhe_bfv_refresh_combine(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_parties, size_t n_cts, const uint8_t crs_seed[32],
                              uint64_t first_index, const uint64_t *c0, const uint64_t *h0, const uint64_t *h1, uint64_t *out0,
                              uint64_t *out1);
/* zkfhe_prof_read slots of the two combine kernels (algorithmic bytes: words read and written); the share products count in
 * ZKFHE_PROF_RNS_NTT and ZKFHE_PROF_RNS_EPILOGUE, the samplers in ZKFHE_PROF_BFV_SAMPLE */
#define ZKFHE_PROF_BFV_PCKS_COMBINE 21      /* k_bfv_pcks_combine */
#define ZKFHE_PROF_BFV_REFRESH_COMBINE 22   /* k_bfv_refresh_combine */

/* ---- BFV slots and rotations on the GPU (bfv_galois.hip) ----
 * SIMD batching and Galois automorphisms.  The conventions above: host arrays, N uint64_t per polynomial in CircuitInput order,
 * residues in [0, Q), the parameter checks of zkfhe_bfv_encrypt; every call waits for its result.  Below, coefficient i is the
 * coefficient of x^i.
 *   sigma_g(m)(x) = m(x^g) mod (x^N + 1), g odd, 1 <= g < 2N: coefficient i moves to k = i g mod 2N, negated (mod Q) and placed at
 *   k - N when k >= N.
 *   Batching: T prime, T < 2^31, 2N | T - 1 (T = 65537 for N <= 32768, 12289 for N <= 2048); then there are N slots.
 *   zeta = r^((T - 1) / 2N) mod T, r the smallest primitive root mod T.  Slot p = row N/2 + j (row in {0, 1}, j < N/2) is the
 *   evaluation at zeta^(e_p), e_p = (-1)^row 5^j mod 2N.  g = 5^k mod 2N rotates both rows left by k (new slot (row, j) = old slot
 *   (row, j + k mod N/2)); g = 2N - 1 swaps the rows.
 *   Galois key of s for g, w = base_bits, l = zkfhe_bfv_relin_digits rows: gk0_i = -(a_i s + e_i) + 2^(i w) sigma_g(s) mod Q,
 *   gk1_i = a_i, a_i uniform from ChaCha20 domain 14 and e_i an error sample from domain 15, both with index g 64 + i (the
 *   samplers of zkfhe_bfv_encrypt).  The key is public; its SEED IS SECRET like any key seed.
 * Slot-encoded plaintexts are ordinary plaintexts (centred residues mod T): zkfhe_bfv_encrypt and the proof take them unchanged, and
 * zkfhe_bfv_mul / zkfhe_bfv_mul_plain multiply them slot by slot.  Every call refuses, with ZKFHE_EINVAL and a message: a NULL
 * argument, n = 0, g even or >= 2N, a coefficient >= Q in a ciphertext or key, a value >= T (encode), a plaintext out of range
 * (decode), a non-ternary sk, base_bits outside [1, 32], and a T that does not batch (encode, decode and zkfhe_bfv_slot_count).
 * Key-switch noise grows with 2^w: a narrower base costs more rows and time and adds less noise. */
/* Host only: *slots = N, or ZKFHE_EINVAL when T is not a batching modulus */
int zkfhe_bfv_slot_count(const zkfhe_bfv_params *params, size_t *slots);
/* Host only: *g = 5^(steps mod N/2) mod 2N (negative steps rotate right), times 2N - 1 mod 2N if swap_rows */
int zkfhe_bfv_galois_element(const zkfhe_bfv_params *params, int64_t steps, int swap_rows, uint64_t *g);
/* Host only: *count = log2(N) and, if g is not NULL, the elements of zkfhe_bfv_slot_sum in order: g = 5^(2^k) mod 2N for
 * k = 0 ... log2(N) - 2, then 2N - 1 */
int zkfhe_bfv_slot_sum_elements(const zkfhe_bfv_params *params, uint64_t *g, size_t *count);
/* n polynomials of N slot values in [0, T) -> the unique m of degree < N over Z_T with m(zeta^(e_p)) = values[p], centred mod T
 * and written as residues mod Q (the representation zkfhe_bfv_decrypt returns).  One LDS NTT mod T per polynomial. */
int zkfhe_bfv_encode_slots(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *values, uint64_t *m_out);
/* the inverse of zkfhe_bfv_encode_slots: n plaintexts in [0, T/2] or [Q - T/2, Q - 1] -> their slot values in [0, T) */
int zkfhe_bfv_decode_slots(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *m, uint64_t *values_out);
/* the Galois key of sk for g (gk0, gk1 of l x N, see above) */
int zkfhe_bfv_galois_keygen(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk, const uint8_t seed[32], uint64_t g,
                            int base_bits, uint64_t *gk0, uint64_t *gk1);
/* n key switches, defined exactly: c'_j = sigma_g(c_j) as residues in [0, Q); digits d_i = (c'_1 >> i w) & (2^w - 1);
 * out0 = c'_0 + sum_i d_i gk0_i, out1 = sum_i d_i gk1_i mod (x^N + 1, Q).  The result decrypts under s to sigma_g(m); g = 1 is a
 * plain key switch.  gk0, gk1: l x N with the same base_bits, transformed once per call. */
int zkfhe_bfv_apply_galois(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1, uint64_t g,
                           const uint64_t *gk0, const uint64_t *gk1, int base_bits, uint64_t *out0, uint64_t *out1);
/* n ciphertexts, each x <- x + zkfhe_bfv_apply_galois(x, g_k) (the sum of zkfhe_bfv_add) for the log2(N) elements of
 * zkfhe_bfv_slot_sum_elements in order, bit for bit that composition; under a batching T every slot then holds the sum of all N
 * slots mod T.  gk0, gk1: log2(N) x l x N, the keys of those elements in the same order, all transformed once per call; the steps
 * run on device buffers. */
int zkfhe_bfv_slot_sum(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1, const uint64_t *gk0,
                       const uint64_t *gk1, int base_bits, uint64_t *out0, uint64_t *out1);
/* party i's share of the collective Galois key for g, in one round (the rotation-key generation of Mouchet et al.):
 * r[j] = -(a_j s_i + e_ij) + 2^(j w) sigma_g(s_i) mod Q, a[j] = a_j; a_j from crs_seed (domain 14), e_ij from party_seed
 * (domain 15), index g 64 + j.  The collective key is gk0 = zkfhe_bfv_share_aggregate of the r_i and gk1 = a; zkfhe_bfv_apply_galois
 * and zkfhe_bfv_slot_sum take it unchanged.  With crs_seed == party_seed == seed, (r, a) is zkfhe_bfv_galois_keygen(seed) bit for
 * bit.  PARTY SEEDS ARE SECRET. */
int zkfhe_bfv_galois_share(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, const uint64_t *sk_i, const uint8_t crs_seed[32],
                           const uint8_t party_seed[32], uint64_t g, int base_bits, uint64_t *r_out, uint64_t *a_out);
/* zkfhe_prof_read slots of the slot and rotation kernels; the CRT epilogue of the key calls (k_rns_epilogue) counts in
 * ZKFHE_PROF_RNS_EPILOGUE */
#define ZKFHE_PROF_BFV_GALOIS 14     /* k_key_switch on sigma_g(c1), k_eval_epilogue of the key switch */
#define ZKFHE_PROF_BFV_SLOT_NTT 15   /* k_slot_ntt */

/* ---- Encrypted matrix-vector products: hoisted rotations and slot-wise linear transforms (bfv_linear.hip) ----
 * out = sum_k diag_k * rot_k(x) for a list of Galois elements, in one call: the digits of c1 are decomposed and transformed once,
 * sigma_g acts on the transforms as an index permutation, and everything stays on the device until the one reduction mod Q.  The
 * conventions of "BFV slots and rotations": host arrays, N uint64_t per polynomial in CircuitInput order, residues in [0, Q), the
 * parameter checks of zkfhe_bfv_encrypt; every call waits for its result; w = base_bits in [1, 32], l = zkfhe_bfv_relin_digits.
 * Galois keys are exactly those of zkfhe_bfv_galois_keygen, or of zkfhe_bfv_share_aggregate over zkfhe_bfv_galois_share; there is
 * no new randomness and no new ChaCha20 domain.
 *   The hoisted rotation of (c0, c1) by g: the digits D_i = (c1 >> i w) & (2^w - 1) are taken from c1 itself, in [0, Q), NOT from
 *   sigma_g(c1).  They are integer polynomials, and sigma_g(D_i) is the signed integer polynomial: the coefficient of x^j moves to
 *   j g mod 2N and is negated over Z when that lands past N.  r1 = sum_i sigma_g(D_i) gk1_i and r0 = sigma_g(c0) + sum_i
 *   sigma_g(D_i) gk0_i, computed exactly over Z in Z[x]/(x^N + 1), then taken mod Q into [0, Q).  For g = 1 the result is (c0, c1)
 *   itself: no key switch, and that element's key rows are neither read nor checked.  The result decrypts under s to sigma_g(m) with
 *   the noise size of zkfhe_bfv_apply_galois, but it is NOT bit-equal to it: the digits of Q - v are not those of v.
 * Range: zkfhe_bfv_linear_transform carries its whole sum in five primes (product 2^151.2) without an intermediate reduction, so it
 * refuses, with ZKFHE_EINVAL and before any device work, when bitlen(n_elems) + bitlen(N) + bitlen(floor(T/2)) + bitlen(Q - 1) +
 * bitlen(1 + l N (2^w - 1)) > 150; the message says to narrow base_bits or to split the element list and add the parts.  At
 * T = 65537 and w <= 16 nothing is refused for any N <= 32768.  zkfhe_bfv_apply_galois_many is bounded by l N 2^w Q < 2^116 and
 * never refuses on range.  Both calls also refuse, with a message: a NULL argument, n = 0 or n_elems = 0, a g that is even or
 * >= 2N, a ciphertext or key coefficient >= Q (the key rows of g = 1 excepted), a diagonal out of plaintext range, base_bits outside
 * [1, 32].  Both are defined for any T.  Noise: every rotated term carries key-switch noise (about l N 2^w B / 2) times the size of
 * its diagonal (up to N T / 2), so keep w small. */
/* out0, out1: n_elems x n x N, element-major; block k is the hoisted rotation of every one of the n ciphertexts by g[k].  g: n_elems
 * odd values below 2N, repeats allowed; gk0, gk1: n_elems x l x N, the key of element k at row block k. */
int zkfhe_bfv_apply_galois_many(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1,
                                size_t n_elems, const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, int base_bits, uint64_t *out0,
                                uint64_t *out1);
/* out0, out1: n x N.  diag: n_elems x N plaintexts in [0, T/2] or [Q - T/2, Q - 1], shared by all n ciphertexts.  With p_k the
 * centred integers of diag_k and (r0_k, r1_k) the hoisted rotation of ciphertext j by g[k]: out_j = sum_k r_{j,k} p_k, exactly over
 * Z in Z[x]/(x^N + 1), then mod Q.  That is, bit for bit, zkfhe_bfv_mul_plain of block k of zkfhe_bfv_apply_galois_many by diag_k,
 * summed over k with zkfhe_bfv_add.  Under a batching T with diag_k = zkfhe_bfv_encode_slots(d_k), slot p of the decryption is
 * sum_k d_k[p] rot_k(v)[p] mod T, rot_k the slot permutation of g[k]. */
int zkfhe_bfv_linear_transform(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1,
                               size_t n_elems, const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, int base_bits,
                               const uint64_t *diag, uint64_t *out0, uint64_t *out1);
/* zkfhe_prof_read slots of the two calls (algorithmic bytes: words read and written); the transforms of the keys and diagonals and
 * the inverse transforms count in ZKFHE_PROF_RNS_NTT, the reduction mod Q in ZKFHE_PROF_BFV_EVAL_EPILOGUE */
#define ZKFHE_PROF_BFV_HOIST 16    /* k_hoist: c0 and the digits of c1, transformed once per ciphertext */
#define ZKFHE_PROF_BFV_LINEAR 17   /* k_linear_acc: the pointwise sums over digits and elements */

/* ---- Baby-step/giant-step linear transforms: dense encrypted matrix products (bfv_linear.hip) ----
 * out = sum_i rot_{G_i}( sum_j diag_{i,j} * rot_{b_j}(x) ) for n_baby baby elements b_j and n_giant giant elements G_i, in one call:
 * n_baby + n_giant Galois keys serve n_baby n_giant diagonals (a dense N x N matrix over the slots: about 2 sqrt(N) keys instead of
 * N), and the whole two-level sum stays on the device between the upload and the download.  The conventions of "Encrypted
 * matrix-vector products": host arrays, N uint64_t per polynomial in CircuitInput order, residues in [0, Q), the parameter checks of
 * zkfhe_bfv_encrypt; the call waits for its result; w = base_bits in [1, 32], l = zkfhe_bfv_relin_digits; Galois keys are those of
 * zkfhe_bfv_galois_keygen, or of zkfhe_bfv_share_aggregate over zkfhe_bfv_galois_share; "hoisted rotation" is the definition above
 * (digits of c1 itself, sigma_g on the signed integer digits).  The result is exact and bit for bit; there is no new randomness and
 * no new ChaCha20 domain.
 *   g_baby: n_baby odd values below 2N with keys bk0, bk1 (n_baby x l x N); g_giant: n_giant odd values below 2N with keys hk0, hk1
 *   (n_giant x l x N); repeats are allowed in both lists; g = 1 in either list is the identity, and its key rows are neither read
 *   nor checked.  diag: n_giant x n_baby x N plaintexts in [0, T/2] or [Q - T/2, Q - 1], giant-major, shared by all n ciphertexts.
 *   For ciphertext x and giant step i, inner_i = zkfhe_bfv_linear_transform(x; g_baby, bk, diag[i]): exact over Z, then mod Q into
 *   [0, Q).  out = sum_i (the hoisted rotation of inner_i by g_giant[i] with key hk[i]), exactly over Z in Z[x]/(x^N + 1), then mod
 *   Q.  That is, bit for bit, the zkfhe_bfv_add-sum over i of block 0 of zkfhe_bfv_apply_galois_many(inner_i, [g_giant[i]]).
 *   diag arrives already pre-rotated: the library does not rotate plaintexts.  Under a batching T with diag[i][j] =
 *   zkfhe_bfv_encode_slots(d'_{i,j}), slot p of the decryption is sum_i sum_j rot_{G_i}(d'_{i,j})[p] rot_{G_i b_j}(v)[p] mod T; for
 *   the diagonal d of the element G_i b_j that means d'_{i,j} = rot_{G_i}^-1(d).
 * Range: the inner sum is carried in five primes as in zkfhe_bfv_linear_transform, so the call refuses, with ZKFHE_EINVAL and before
 * any pass over the inputs and any device work, when bitlen(n_baby) + bitlen(N) + bitlen(floor(T/2)) + bitlen(Q - 1) + bitlen(1 + l N
 * (2^w - 1)) > 150, with that call's message.  The outer sum is over rotations of inner ciphertexts in [0, Q): it is below n_giant Q
 * (1 + l N (2^w - 1)) < 2^20 2^63 2^49 = 2^132 and never needs a refusal.  The call also refuses, with a message: a NULL argument;
 * n, n_baby or n_giant equal to 0; either count >= 2^20; a g that is even or >= 2N; a ciphertext or key coefficient >= Q (the key
 * rows of g = 1 excepted); a diagonal out of plaintext range; base_bits outside [1, 32].  Defined for any T.  Noise: the inner sum
 * has the noise of zkfhe_bfv_linear_transform over n_baby elements, and every giant step adds one more key switch (about l N 2^w B /
 * 2) that no diagonal multiplies. */
/* out0, out1: n x N. */
int zkfhe_bfv_linear_transform_bsgs(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1,
                                    size_t n_baby, const uint64_t *g_baby, const uint64_t *bk0, const uint64_t *bk1,
                                    size_t n_giant, const uint64_t *g_giant, const uint64_t *hk0, const uint64_t *hk1, int base_bits,
                                    const uint64_t *diag, uint64_t *out0, uint64_t *out1);
/* zkfhe_prof_read slots of the call's own kernels (algorithmic bytes: words read and written); k_hoist and the baby rotations count
 * in ZKFHE_PROF_BFV_HOIST and ZKFHE_PROF_BFV_LINEAR, the transforms in ZKFHE_PROF_RNS_NTT, the reductions mod Q in
 * ZKFHE_PROF_BFV_EVAL_EPILOGUE */
#define ZKFHE_PROF_BFV_BSGS_INNER 18   /* k_bsgs_inner: the pointwise products of the diagonals with the baby rotations */
#define ZKFHE_PROF_BFV_BSGS_GIANT 19   /* k_linear_acc<ACC_GIANT>: the giant rotations of the inner sums, accumulated */

/* ---- Prepared plans: a linear transform's keys and diagonals kept on the device (bfv_linear.hip) ----
 * zkfhe_bfv_linear_transform and zkfhe_bfv_linear_transform_bsgs check, upload and forward-transform every Galois key and every
 * diagonal on every call.  A plan does that once: it is opaque, immutable and device-resident, and holds exactly what those calls
 * build before they touch a ciphertext (the element table, the transformed keys, the transformed diagonals; params, base_bits, l
 * and the counts), not the untransformed copies.  zkfhe_bfv_plan_apply is the rest of the call.
 * Exactness: zkfhe_bfv_plan_apply on a plan of zkfhe_bfv_plan_create returns, bit for bit, zkfhe_bfv_linear_transform of the same
 * ciphertexts with the plan's arguments; on a plan of zkfhe_bfv_plan_create_bsgs, bit for bit, zkfhe_bfv_linear_transform_bsgs:
 * for every n, across ciphertext chunks and groups of giant steps, and with the same kernels.  No new arithmetic is defined; there
 * is no new randomness and no new ChaCha20 domain.  g = 1 keeps its meaning: its key rows are neither read nor checked, and it
 * takes no key slot.  The conventions are those of the two calls (host arrays, N uint64_t per polynomial in CircuitInput order).
 * Refusals at creation are those of the host-array call that do not concern ciphertexts, in that call's order and with its texts,
 * under the prefix "bfv_plan_create:" / "bfv_plan_create_bsgs:" (bad parameters: the text of every BFV call): a NULL argument, a
 * zero count or bad parameters; base_bits outside [1, 32]; a count >= 2^20; a g that is even or >= 2N; the 150-bit range rule
 * (over n_elems, or over n_baby), before any pass over the inputs and any device work; a key coefficient >= Q (the key rows of g = 1
 * excepted); a diagonal out of plaintext range.  On any failure, a failed allocation (ZKFHE_ENOMEM) included, everything allocated
 * so far is freed and *out is NULL.
 * Refusals at apply, under the prefix "bfv_plan_apply:": a NULL argument or n = 0; a context on another device than the plan's; a
 * ciphertext coefficient >= Q.  No output is written in any of these cases.
 * Ownership: the plan's buffers are device allocations of its own, not part of a context's workspace (which the next call
 * reuses), and live until zkfhe_bfv_plan_destroy.  Creation waits for its device work, and the plan is read-only afterwards, so
 * any context of the same device may apply it, each with its own workspace and from its own thread.  zkfhe_bfv_plan_destroy waits
 * for the context it is given and then frees; destroying a plan that another context is still applying is the caller's error.
 * device_bytes of zkfhe_bfv_plan_info and zkfhe_bfv_plan_bytes are the sum of the sizes requested from the device:
 * 4 (2 n_elems_total + 2 n_key_slots l N 5 + n_diagonals N 5) with l = zkfhe_bfv_relin_digits, n_elems_total = n_elems or n_baby +
 * n_giant, n_diagonals = n_elems or n_baby n_giant.  The dense N = 1024 matrix at a 60-bit Q and w = 8 (l = 8; 32 x 32 elements,
 * 62 key slots): 512 + 20316160 + 20971520 = 41288192 bytes. */
typedef struct zkfhe_bfv_plan zkfhe_bfv_plan;
/* flat: the arguments of zkfhe_bfv_linear_transform without the ciphertexts */
int zkfhe_bfv_plan_create(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_elems, const uint64_t *g, const uint64_t *gk0,
                          const uint64_t *gk1, int base_bits, const uint64_t *diag, zkfhe_bfv_plan **out);
/* two-level: the arguments of zkfhe_bfv_linear_transform_bsgs without the ciphertexts */
int zkfhe_bfv_plan_create_bsgs(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_baby, const uint64_t *g_baby, const uint64_t *bk0,
                               const uint64_t *bk1, size_t n_giant, const uint64_t *g_giant, const uint64_t *hk0, const uint64_t *hk1,
                               int base_bits, const uint64_t *diag, zkfhe_bfv_plan **out);
/* n ciphertexts through the plan: c0, c1, out0, out1 host arrays n x N; waits for its result, like every evaluation call.  The
 * zkfhe_prof_read slots are those of the host-array call, less the transforms of the keys and the diagonals. */
int zkfhe_bfv_plan_apply(zkfhe_ctx *ctx, const zkfhe_bfv_plan *plan, size_t n, const uint64_t *c0, const uint64_t *c1, uint64_t *out0,
                         uint64_t *out1);
/* host only; any output pointer may be NULL.  counts = { n_elems (flat) or n_baby, n_giant (0 for a flat plan), the key slots (the
 * elements with g != 1) } */
int zkfhe_bfv_plan_info(const zkfhe_bfv_plan *plan, zkfhe_bfv_params *params, int *base_bits, size_t counts[3], uint64_t *device_bytes);
/* host only: what a plan will hold, so that a service can budget its HBM before it creates one.  Refuses bad parameters and
 * base_bits outside [1, 32]. */
int zkfhe_bfv_plan_bytes(const zkfhe_bfv_params *params, int base_bits, size_t n_elems_total, size_t n_key_slots, size_t n_diagonals,
                         uint64_t *bytes);
/* waits for ctx (a context of the plan's device), then frees the plan; a NULL plan is not an error */
int zkfhe_bfv_plan_destroy(zkfhe_ctx *ctx, zkfhe_bfv_plan *plan);

/* ---- The ballot box: from verified proofs to a tally (bfv_ballot.hip) ----
 * The joint between zkfhe_bfv_verify_batch and zkfhe_bfv_sum.  A proof's public inputs ("instances") are 5 N + 1 canonical 32-byte
 * little-endian scalars pk0 | pk1 | c0 | c1 | cyclo; position p of a polynomial's N scalars is word p of its N uint64_t in
 * CircuitInput order, so the low limb of scalar 2 N + p is c0[p] and that of scalar 3 N + p is c1[p].
 * An item IS A CIPHERTEXT only if all three hold: it has exactly 5 N + 1 scalars; each of the 2 N scalars of c0 | c1 (positions
 * 2 N ... 4 N - 1) has limbs 1 to 3 zero and limb 0 below Q; the last N + 1 scalars spell x^N + 1 highest degree first, that is
 * 1, 0, ..., 0, 1.  Per-item statuses (int32_t; one total per status, ZKFHE_BALLOT_STATUSES of them, in zkfhe_bfv_box_info): */
#define ZKFHE_BALLOT_COUNTED 0            /* summed into its group */
#define ZKFHE_BALLOT_SKIPPED 1            /* zkfhe_bfv_sum_instances: group < 0 */
#define ZKFHE_BALLOT_BAD_GROUP 2          /* group >= n_groups (the box: also group < 0) */
#define ZKFHE_BALLOT_NOT_A_CIPHERTEXT 3   /* one of the three conditions above fails */
#define ZKFHE_BALLOT_WRONG_KEY 4          /* the box: pk0 | pk1 is not the box's key */
#define ZKFHE_BALLOT_REJECTED 5           /* the box: zkfhe_bfv_verify_batch rejects the proof */
#define ZKFHE_BALLOT_REPEATED 6           /* the box: c0 | c1 equals that of a ballot already counted */
#define ZKFHE_BALLOT_STATUSES 7
/* Host only.  The four polynomials of one item: the three conditions, with the second one applied to all 4 N scalars of
 * pk0 | pk1 | c0 | c1.  *status = ZKFHE_BALLOT_COUNTED and the low limbs written to pk0, pk1, c0, c1 (N words each; any may be NULL),
 * or *status = ZKFHE_BALLOT_NOT_A_CIPHERTEXT and nothing written; both return ZKFHE_OK.  With status == NULL an item that is not a
 * ciphertext is ZKFHE_EINVAL.  Refused with ZKFHE_EINVAL and a message "bfv_instances_unpack: ...": NULL params or instances; bad
 * parameters (the text of every BFV call).  What it returns feeds zkfhe_bfv_mul, zkfhe_bfv_dot and the plans. */
int zkfhe_bfv_instances_unpack(const zkfhe_bfv_params *params, const uint8_t *instances, size_t n_instances, uint64_t *pk0, uint64_t *pk1,
                               uint64_t *c0, uint64_t *c1, int32_t *status);
/* Sums straight from instance scalars, WITHOUT verification: item j has n_instances[j] scalars at instances[j] and belongs to group
 * group[j] (group == NULL: every item to group 0).  Defined exactly: out0[g], out1[g] (N words each, [n_groups][N]) are the sums mod Q,
 * coefficient-wise, of the c0 / c1 words of the items with group[j] == g that are ciphertexts; an empty group is all zeros;
 * counted[g] is the number of items summed into group g.  status[j], decided in this order: ZKFHE_BALLOT_SKIPPED (group[j] < 0),
 * ZKFHE_BALLOT_BAD_GROUP (group[j] >= n_groups), ZKFHE_BALLOT_NOT_A_CIPHERTEXT, ZKFHE_BALLOT_COUNTED.  A malformed item never
 * contributes and never fails the call.  Only the c0 | c1 span of an item goes to the device, in chunks (k_ballot_unpack checks and
 * unpacks it, k_ballot_sum adds it to its group); the count and the cyclotomic tail are compared on the host.
 * Refused with ZKFHE_EINVAL and a message "bfv_sum_instances: ...", in this order and before any device work: a NULL argument other
 * than ctx and group (an instances[j] with n_instances[j] > 0 included) or n_items = 0; n_groups outside [1, 4096]; bad parameters
 * (the text of every BFV call); a NULL ctx.  Waits for its result. */
int zkfhe_bfv_sum_instances(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_items, const uint8_t *const *instances,
                            const size_t *n_instances, const int32_t *group, size_t n_groups, uint64_t *out0, uint64_t *out1,
                            uint64_t *counted, int32_t *status);
/* The box: a device-resident tally that takes (instances, proof) pairs and counts exactly the ones that deserve it.  It owns a copy
 * of the vk bytes, of the verifier's half of the SRS (srs_seed, or g2 and s_g2: the convention of zkfhe_bfv_verify_batch), of the
 * election's public key pk0 | pk1 (N words each, below Q) and of the parameters.  On the device, from create to destroy: the
 * accumulator [n_groups][2][N], the counts per group and the totals per status.  On the host: the set of the Blake2b-256 digests
 * (no personalisation) of the 2 N little-endian words c0 | c1 of every ballot counted so far.
 * zkfhe_bfv_box_add decides the fate of proof j in this fixed order (group == NULL: every proof to group 0):
 *   1. ZKFHE_BALLOT_BAD_GROUP         group[j] outside [0, n_groups): a negative group is bad here, not skipped
 *   2. ZKFHE_BALLOT_NOT_A_CIPHERTEXT  n_instances[j] != 5 N + 1, or a wrong cyclotomic tail
 *   3. ZKFHE_BALLOT_WRONG_KEY         the first 2 N scalars are not the box's pk0 | pk1
 *   4. ZKFHE_BALLOT_REJECTED          the remaining proofs, and only those, go through zkfhe_bfv_verify_batch in one call; for a
 *                                     proof it rejects, errs + j * err_stride holds the reason exactly as zkfhe_bfv_verify words it
 *   5. ZKFHE_BALLOT_NOT_A_CIPHERTEXT  an accepted proof whose c0 | c1 is not made of residues below Q (the device check)
 *   6. ZKFHE_BALLOT_REPEATED          c0 | c1 equals that of a ballot counted earlier in this box, in an earlier call or earlier in
 *                                     this one; the group plays no part
 *   7. ZKFHE_BALLOT_COUNTED           the ciphertext is summed into its group
 * Only ACCEPTED proofs enter the digest set, so a forged proof that carries a copied ciphertext can never shut out the genuine
 * ballot; within a call the first accepted occurrence wins.  The tally does not depend on how the ballots were split into calls or on
 * their order; only WHICH copy of a repeat is flagged does.  errs may be NULL; every other reason is the empty string.
 * zkfhe_bfv_box_tally downloads the accumulator (out0, out1: [n_groups][N]) and the counts ([n_groups]); it does not change the box
 * and may be called between adds.  zkfhe_bfv_box_info is host only (it reports the box's host mirror of the device totals and touches
 * no device); any output may be NULL; totals[s] is the number of proofs that ended with status s over all completed adds.
 * Refused with ZKFHE_EINVAL and a message "bfv_box: ...": create: a NULL argument other than ctx, srs_seed, g2 and s_g2, or vk_len = 0;
 * n_groups outside [1, 4096]; bad parameters (the text of every BFV call); only one of g2 and s_g2, or a NULL srs_seed with a length;
 * a NULL ctx; a public-key coefficient >= Q.  add: a NULL argument other than group and errs (a proofs[j] or instances[j] with a
 * non-zero length included) or n_proofs = 0.  tally: a NULL argument.  add and tally: a context of another device than the box's.
 * If an error interrupts the summing of an add once its first device command is issued, the call returns it and the box refuses every
 * later add and tally with a message that says so: a tally that may be half-applied is never handed out.  A failure before that (the
 * verifier's, or no room for the work buffers) leaves the box as it was.  One add at a time per box is the caller's duty, as for
 * contexts; any context of the box's device may add, tally and destroy.  zkfhe_bfv_box_destroy waits for ctx, then frees; a NULL box is
 * not an error. */
typedef struct zkfhe_bfv_box zkfhe_bfv_box;
int zkfhe_bfv_box_create(zkfhe_ctx *ctx, const uint8_t *vk_bytes, size_t vk_len, const zkfhe_bfv_params *params, const uint64_t *pk0,
                         const uint64_t *pk1, size_t n_groups, const uint8_t *srs_seed, size_t seed_len, const uint8_t *g2,
                         const uint8_t *s_g2, zkfhe_bfv_box **out);
int zkfhe_bfv_box_add(zkfhe_ctx *ctx, zkfhe_bfv_box *box, size_t n_proofs, const uint8_t *const *instances, const size_t *n_instances,
                      const uint8_t *const *proofs, const size_t *proof_lens, const int32_t *group, int32_t *status, char *errs,
                      size_t err_stride);
int zkfhe_bfv_box_tally(zkfhe_ctx *ctx, const zkfhe_bfv_box *box, uint64_t *out0, uint64_t *out1, uint64_t *counted);
int zkfhe_bfv_box_info(const zkfhe_bfv_box *box, zkfhe_bfv_params *params, size_t *n_groups, uint64_t totals[ZKFHE_BALLOT_STATUSES]);
int zkfhe_bfv_box_destroy(zkfhe_ctx *ctx, zkfhe_bfv_box *box);
/* zkfhe_prof_read slot of the ballot kernels */
#define ZKFHE_PROF_BFV_BALLOT 24   /* k_ballot_unpack, k_ballot_sum (and the few-thread k_ballot_totals of the box) */

/* ---- Resident ciphertext batches: chaining evaluation calls on the device (bfv_resident.hip) ----
 * Every evaluation call above takes host arrays: it checks them on the host, uploads them, runs a few kernels, downloads the result
 * and waits.  A batch keeps ciphertexts on the device between calls: it is opaque and holds n ciphertexts as two planes c0[n][N]
 * and c1[n][N] (N uint64_t per polynomial, CircuitInput order) in one device allocation of its own, with its parameters and its
 * device.  The calls below are the evaluation calls on batches.  No new arithmetic is defined, there is no new randomness and no new
 * ChaCha20 domain.
 * INVARIANT: every word of a batch is a residue below Q, from creation to destruction.  Every way in either checks this or preserves
 * it: zkfhe_bfv_cts_alloc writes zeros; zkfhe_bfv_cts_upload and zkfhe_bfv_cts_store check on the device (k_cts_check, one pass,
 * one flag word read once) before a word becomes part of a batch; every other call writes residues that a kernel computed mod Q from
 * residues.  Calls on batches therefore run no range pass over ciphertexts; the host arrays of a call (plaintexts, keys, indices,
 * groups) are checked on the host as in the host-array call.
 * Ownership: the allocation is the batch's own, not part of a context's workspace (which the next call reuses), and lives until
 * zkfhe_bfv_cts_destroy.  Any context of the same device may use a batch; a context of another device is refused ("...: the batch
 * lives on device D and the context on device E").  Every call waits for its result, like every evaluation call, so a batch used by
 * two contexts needs no stream bookkeeping; two calls at once on one batch, one of them writing, are the caller's error.
 * zkfhe_bfv_cts_destroy waits for the context it is given and then frees.
 * Evaluation: every call writes into a caller-provided destination batch dst of the right count and allocates no device memory
 * (freeing it would synchronise the device and stall a prover running beside it).  Sources and dst share parameters and device.
 *   call                                                      definition (bit for bit)                       dst may be a source
 *   zkfhe_bfv_cts_add(ctx, a, b, subtract, dst)               zkfhe_bfv_add                                  yes
 *   zkfhe_bfv_cts_add_plain(ctx, a, m_count, m, dst)          zkfhe_bfv_add_plain; m a host array            yes
 *   zkfhe_bfv_cts_mul_plain(ctx, a, m_count, m, dst)          zkfhe_bfv_mul_plain; m a host array            yes
 *   zkfhe_bfv_cts_mul(ctx, a, b, rlk0, rlk1, base_bits, dst)  zkfhe_bfv_mul; the key host arrays, checked    yes
 *                                                             and transformed once per call
 *   zkfhe_bfv_cts_apply_galois(ctx, a, g, gk0, gk1,           zkfhe_bfv_apply_galois; the key host arrays    yes
 *                              base_bits, dst)
 *   zkfhe_bfv_cts_plan_apply(ctx, plan, a, dst)               zkfhe_bfv_plan_apply; the plan's parameters    yes
 *                                                             equal the batch's
 *   zkfhe_bfv_cts_select(ctx, a, n_idx, idx, dst)             dst[j] = a[idx[j]], j < n_idx = dst's count;   no (refused)
 *                                                             idx a host array, repeats allowed: slice,
 *                                                             reorder, broadcast (k_cts_gather)
 *   zkfhe_bfv_cts_sum(ctx, a, group, n_groups, dst)           dst[g] = zkfhe_bfv_sum of the members with     no (refused)
 *                                                             group[j] == g (k_cts_group_sum)
 * "Bit for bit": downloading dst gives exactly what the host-array call returns on the downloaded sources, for every n, across
 * ciphertext chunks, and with the same kernels: each host-array call is a wrapper (host checks, uploads, downloads) around a device
 * core on device pointers, and the batch call drives the same core from resident memory, so the zkfhe_prof_read slots of a batch
 * call are those of the host-array call.
 * Alias rules: where the table says yes, dst may be a or b (or both).  A chunk's result goes to the context's workspace and is copied
 * into dst after the kernels that read the chunk, on the same stream, so a chunk is read completely before it is written.
 * zkfhe_bfv_cts_sum: group is a host array of a's count (NULL: everything to group 0); group[j] < 0 is skipped; an empty group is all
 * zeros; n_groups is in [1, 4096] and dst holds n_groups ciphertexts.  The member lists are built on the host; every thread owns
 * output coefficients and adds its group's members in the order of the batch.  Addition mod Q is exact, so the result equals any
 * order of zkfhe_bfv_add; no atomics and no floating point are involved.
 * Refusals: ZKFHE_EINVAL with a message "bfv_cts_<name>: ..." (zkfhe_bfv_box_tally_cts: "bfv_cts_box_tally: ...", and the box's own
 * refusals under "bfv_box: ..."), in this order and all before any device work on ciphertexts: a NULL argument, a zero count or bad
 * parameters (the text of every BFV call); a batch (or plan) on another device than the context's; batches of different parameters,
 * or a count that does not match (b and dst hold a's count; dst of select holds n_idx, dst of sum n_groups); dst among the sources
 * where the table says no; an index >= a's count, a group >= n_groups, a range of store / download outside the batch; then the key
 * and plaintext checks of the host-array call with its texts (base_bits outside [1, 32], g even or >= 2N, m_count neither 1 nor the
 * count, a key coefficient >= Q, a plaintext out of range).  A refused call leaves dst as it was.
 * zkfhe_bfv_cts_upload: allocates, uploads in chunks, checks; on a coefficient >= Q ("bfv_cts_upload: a ciphertext coefficient >= Q")
 * or any other failure (ZKFHE_ENOMEM included) everything is freed and *out is NULL.  zkfhe_bfv_cts_store is the same checked upload
 * into ciphertexts first ... first + count - 1 of an existing batch: every chunk is staged and checked before the batch is touched,
 * so a refused store leaves the batch as it was.  zkfhe_bfv_cts_info is host only; any output may be NULL; device_bytes = 16 n N.
 * zkfhe_bfv_box_tally_cts copies the box's accumulator into dst (n_groups ciphertexts with the box's parameters) without touching
 * the host; counted is as in zkfhe_bfv_box_tally, and the box is unchanged. */
typedef struct zkfhe_bfv_cts zkfhe_bfv_cts;
/* n ciphertexts of zero */
int zkfhe_bfv_cts_alloc(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, zkfhe_bfv_cts **out);
/* c0, c1: host arrays n x N */
int zkfhe_bfv_cts_upload(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1,
                         zkfhe_bfv_cts **out);
int zkfhe_bfv_cts_store(zkfhe_ctx *ctx, zkfhe_bfv_cts *cts, size_t first, size_t count, const uint64_t *c0, const uint64_t *c1);
/* out0, out1: host arrays count x N */
int zkfhe_bfv_cts_download(zkfhe_ctx *ctx, const zkfhe_bfv_cts *cts, size_t first, size_t count, uint64_t *out0, uint64_t *out1);
int zkfhe_bfv_cts_info(const zkfhe_bfv_cts *cts, zkfhe_bfv_params *params, size_t *n, uint64_t *device_bytes);
/* waits for ctx (a context of the batch's device; may be NULL), then frees the batch; a NULL batch is not an error */
int zkfhe_bfv_cts_destroy(zkfhe_ctx *ctx, zkfhe_bfv_cts *cts);
int zkfhe_bfv_box_tally_cts(zkfhe_ctx *ctx, const zkfhe_bfv_box *box, zkfhe_bfv_cts *dst, uint64_t *counted);
int zkfhe_bfv_cts_add(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, int subtract, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_add_plain(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t m_count, const uint64_t *m, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_mul_plain(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t m_count, const uint64_t *m, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_mul(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, const uint64_t *rlk0, const uint64_t *rlk1,
                      int base_bits, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_apply_galois(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, uint64_t g, const uint64_t *gk0, const uint64_t *gk1, int base_bits,
                               zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_plan_apply(zkfhe_ctx *ctx, const zkfhe_bfv_plan *plan, const zkfhe_bfv_cts *a, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_select(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t n_idx, const uint64_t *idx, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_sum(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const int32_t *group, size_t n_groups, zkfhe_bfv_cts *dst);
/* zkfhe_prof_read slot of the batches' own kernels: algorithmic bytes = the words read and written.  The evaluation calls on batches
 * count in the slots of their host-array calls. */
#define ZKFHE_PROF_BFV_RESIDENT 25   /* k_cts_check, k_cts_gather, k_cts_group_sum */

/* ---- Evaluation keys that stay on the device: slot sums and inner products on batches (bfv_evk.hip, bfv_resident.hip, bfv_key_switch.hip) ----
 * zkfhe_bfv_cts_mul and zkfhe_bfv_cts_apply_galois take their keys as host arrays and check, upload and transform them on every
 * call.  A key set keeps one relinearization key and any number of Galois keys on the device: it is opaque and holds, for the
 * relinearization key (if any) and then for each Galois key in the order of g, the [2 l][5][N] uint32_t transform that the key
 * switch reads (l = zkfhe_bfv_relin_digits), in one device allocation of its own: device_bytes = (has_relin + n_galois) 2 l 5 N 4 =
 * zkfhe_bfv_evk_bytes.  No new arithmetic is defined, there is no new randomness and no new ChaCha20 domain.
 * zkfhe_bfv_evk_create: rlk0, rlk1 are [l][N] or both NULL; g holds n_galois elements and gk0, gk1 are [n_galois][l][N] (n_galois
 * may be 0, but not beside a NULL relinearization key).  It runs the host checks of the host-array calls with their texts under
 * "bfv_evk_create: ...": a NULL argument; neither key ("... neither a relinearization key nor a Galois key"); bad parameters;
 * base_bits outside [1, 32]; a g even or >= 2N; a g given twice ("... the Galois element G is repeated"); a key coefficient >= Q.
 * Then it uploads the keys in chunks through the context's workspace and transforms them straight into the set, so the stored
 * words are exactly those a host-array call computes from the same key.  On any failure (ZKFHE_ENOMEM included) everything is freed
 * and *out is NULL.  The set is read-only and complete when the call returns: any context of the same device may use it, a context of
 * another device is refused ("...: the key set lives on device D and the context on device E").  zkfhe_bfv_evk_info and
 * zkfhe_bfv_evk_bytes are host only; any output of info may be NULL, g_out takes n_galois elements.  zkfhe_bfv_evk_destroy waits
 * for the context it is given and then frees.
 * The calls on batches that take a set follow the conventions of "Resident ciphertext batches": dst is caller-provided, nothing is
 * allocated on the device, every call waits for its result, a refused call leaves dst as it was.
 *   call                                                  definition (bit for bit)                              dst may be a source
 *   zkfhe_bfv_cts_mul_evk(ctx, a, b, evk, dst)            zkfhe_bfv_mul with the set's relinearization key      yes
 *   zkfhe_bfv_cts_apply_galois_evk(ctx, a, g, evk, dst)   zkfhe_bfv_apply_galois with the set's key for g       yes
 *   zkfhe_bfv_cts_slot_sum(ctx, a, evk, dst)              zkfhe_bfv_slot_sum with the set's keys for the        yes
 *                                                         elements of zkfhe_bfv_slot_sum_elements
 *   zkfhe_bfv_cts_dot(ctx, a, b, n_terms, evk, dst)       zkfhe_bfv_dot: n_groups = dst's count, a holds        no (refused)
 *                                                         n_groups n_terms ciphertexts in [group][term] order,
 *                                                         b n_terms (shared) or n_groups n_terms
 *   zkfhe_bfv_cts_dot_plain(ctx, a, n_terms, m_groups,    zkfhe_bfv_dot_plain: a as for dot; m a host array of  no (refused)
 *                           m, dst)                       m_groups n_terms plaintexts; takes no key set
 * Alias rules: where the table says yes, dst may be a or b (or both); a chunk is read completely before it is written.
 * Refusals: ZKFHE_EINVAL with a message "bfv_cts_<name>: ...", in this order and all before any device work: a NULL argument or a
 * zero count; a batch on another device; the key set on another device; "the key set and the batch have different parameters";
 * batches of different parameters; a count that does not fit ("X holds H ciphertexts and the call needs W"); dst among the sources
 * where the table says no ("dst must not be a source"); g even or >= 2N; "the key set has no relinearization key"; "the key set
 * has no key for the Galois element G"; m_groups neither 1 nor n_groups; n_terms above zkfhe_bfv_dot_max_terms, with the text of
 * zkfhe_bfv_dot; a plaintext out of range.
 * The digit-parallel key switch.  The key switch of the host-array calls (k_key_switch) runs one workgroup per (ciphertext, prime)
 * that walks the l digits one after the other: 5 workgroups for one ciphertext.  The calls above run, where l >= 2 and a chunk
 * holds at most zkfhe_bfv_evk_wide_max ciphertexts, k_key_switch_digit (one workgroup per (digit, ciphertext, prime): the digit
 * transformed and multiplied by its two key rows into partials in the workspace) and k_key_switch_fold (one workgroup per
 * (component, ciphertext, prime): the l partials summed mod p, one inverse transform).  Both ways share the digit load and the
 * product with the key rows, and a sum of canonical residues mod p does not depend on its order, so the result is bit for bit that
 * of k_key_switch.  The bound keeps the grid of
 * k_key_switch_digit, 5 l workgroups per ciphertext, at or below 5/4 of the device's CU count (16 ciphertexts at l = 4 on 256 CUs)
 * and the partials within the accumulators a full chunk already needs;
 * profiles/bfv_evk.md holds the measurement behind it (for which alone the environment variable ZKFHE_EVK_WIDE_MAX, read once per
 * process, replaces the first of the two limits by a count).  The calls of the earlier sections never take this path: their
 * kernels and launch counts are unchanged. */
typedef struct zkfhe_bfv_evk zkfhe_bfv_evk;
int zkfhe_bfv_evk_create(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, int base_bits, const uint64_t *rlk0, const uint64_t *rlk1,
                         size_t n_galois, const uint64_t *g, const uint64_t *gk0, const uint64_t *gk1, zkfhe_bfv_evk **out);
int zkfhe_bfv_evk_bytes(const zkfhe_bfv_params *params, int base_bits, int has_relin, size_t n_galois, uint64_t *bytes);
int zkfhe_bfv_evk_info(const zkfhe_bfv_evk *evk, zkfhe_bfv_params *params, int *base_bits, int *has_relin, size_t *n_galois,
                       uint64_t *g_out, uint64_t *device_bytes);
/* waits for ctx (a context of the set's device; may be NULL), then frees the set; a NULL set is not an error */
int zkfhe_bfv_evk_destroy(zkfhe_ctx *ctx, zkfhe_bfv_evk *evk);
/* the largest count of ciphertexts in a chunk that takes the digit-parallel key switch on this device (0: never, as for l = 1) */
int zkfhe_bfv_evk_wide_max(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, int base_bits, size_t *c_max);
int zkfhe_bfv_cts_mul_evk(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_apply_galois_evk(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, uint64_t g, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_slot_sum(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_dot(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, const zkfhe_bfv_cts *b, size_t n_terms, const zkfhe_bfv_evk *evk,
                      zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_dot_plain(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t n_terms, size_t m_groups, const uint64_t *m, zkfhe_bfv_cts *dst);
/* zkfhe_prof_read slot of the digit-parallel key switch: algorithmic bytes = the words read and written.  Everything else a call
 * with a key set launches counts in the slots of its host-array call; no such call launches a key transform. */
#define ZKFHE_PROF_BFV_KEY_SWITCH_WIDE 26   /* k_key_switch_digit, k_key_switch_fold */

/* ---- Evaluation keys modulo Q P: hybrid key switching (bfv_hybrid.hip, bfv_evk.hip) ----
 * The key switch of the sections above adds the key errors times the digits, about l N 2^w B of noise.  A hybrid key set
 * (Gentry-Halevi-Smart) keeps its keys modulo Q P for a special modulus P that no ciphertext ever sees, scales the gadget by P and
 * divides the sum over the digits by P, with rounding, before it is added: the added noise is at most
 * ceil(l N (2^w - 1) B / P) + (N + 1) / 2 for a ternary key.  Hybrid keys are a property of a resident key set: a set made by
 * zkfhe_bfv_evk_create_hybrid is taken by zkfhe_bfv_cts_mul_evk, zkfhe_bfv_cts_apply_galois_evk, zkfhe_bfv_cts_slot_sum,
 * zkfhe_bfv_cts_dot and zkfhe_bfv_cts_pack with their signatures, refusals and alias rules unchanged.
 * Special modulus: 2 <= P < 2^63, gcd(P, Q) = 1 and l N (2^w - 1) (Q P - 1) <= floor(P5 / 2), with l = zkfhe_bfv_relin_digits(w) and
 * P5 the product of the five RNS primes (2^151.2); P need not be prime.  zkfhe_bfv_hybrid_max_p (host only) returns the largest P
 * below 2^63 that meets the bound; it ignores the gcd condition and is never below 2^34 for admissible parameters.
 * A hybrid key has rows K0_i, K1_i, i < l, each a polynomial of integers in [0, Q P).  It is passed as two planes of [l][N] words
 * each, in the conventions of the ordinary keys: the q-plane K mod Q (coefficients below Q) and the p-plane K mod P (coefficients
 * below P); K is the unique integer below Q P with those two residues.
 * Hybrid key switch of a source polynomial v (residues in [0, Q), exactly what the ordinary key switch decomposes):
 *   d_i = (v >> i w) & (2^w - 1);  X_j = sum_i d_i Kj_i exactly over Z in Z[x]/(x^N + 1), j = 0, 1;
 *   r_j = floor((2 X_j + P) / 2P) mod Q coefficient-wise: to nearest, ties upward, a true floor for negative X_j.
 * Wherever the definition of a call says sum_i d_i key0_i and sum_i d_i key1_i mod Q, a hybrid set puts r_0 and r_1; every other
 * word of the definitions of mul, dot, apply_galois, slot_sum and pack stands.
 * Keys (w = base_bits; s ternary, lifted to {-1, 0, 1}; e_i the centred error integer of the error sampler, the same integer in
 * both planes, which needs 2 B < Q: "...: B must be below Q / 2" otherwise):
 *   relinearization key   q-plane  K0_i = -(aQ_i s + e_i) + (P mod Q) 2^(i w) s^2 mod Q,  K1_i = aQ_i
 *                         p-plane  K0_i = -(aP_i s + e_i) mod P,                          K1_i = aP_i
 *     aQ_i, e_i: the a_i, e_i of zkfhe_bfv_relin_keygen (domains 7 and 8, index i); aP_i: ChaCha20 domain 23, index i, the uniform
 *     sampler with P in place of Q
 *   Galois key for g      the same with sigma_g(s) in place of s^2; aQ_i, e_i from domains 14 and 15, index g 64 + i; aP_i from
 *     domain 24 with the same index.  As in zkfhe_bfv_galois_share, the a come from crs_seed and the e from party_seed;
 *     zkfhe_bfv_galois_keygen_hybrid is the share with crs_seed = party_seed = seed, bit for bit.
 * Domains 1 to 22 keep their meaning; the new ones are 23 (aP_i of the relinearization key) and 24 (aP_i of a Galois key).
 * A committee's hybrid Galois key is formed from the planes separately: gk0_q = zkfhe_bfv_share_aggregate of the r_q shares as
 * today, gk0_p = the same call on the r_p shares under parameters whose q is P (the parameter check then asks 2 <= T < P and
 * 1 <= B < min(P, 1024) of them, which T = 2, B = 1 meet for every P >= 3; the sum does not read T or B); gk1_q = a_q, gk1_p = a_p.
 * zkfhe_bfv_evk_create_hybrid: the arguments of zkfhe_bfv_evk_create with P and a p-plane beside every q-plane.  The words of a
 * hybrid set have the layout of an ordinary one ([keys][2 l][5][N]: the transform of K mod p_j, formed from the planes by Garner,
 * t = (kp - kq) Q^-1 mod P, K = kq + Q t), so zkfhe_bfv_evk_bytes holds for both and zkfhe_bfv_evk_info is unchanged.
 * zkfhe_bfv_evk_special_modulus gives P, and 1 for an ordinary set.  Refusals: ZKFHE_EINVAL with a message "bfv_evk_create_hybrid:
 * ..." (the key generators: "bfv_relin_keygen_hybrid: ...", "bfv_galois_keygen_hybrid: ...", "bfv_galois_share_hybrid: ..."), in
 * this order and before any device work: a NULL argument or nothing to hold, as zkfhe_bfv_evk_create; bad parameters or base_bits;
 * "... P must satisfy 2 <= P < 2^63"; "... P and Q must be coprime"; "... P is above the limit L of zkfhe_bfv_hybrid_max_p"; the
 * checks on g of the ordinary call; a q-plane word >= Q (the texts of zkfhe_bfv_evk_create); a p-plane word >= P ("... a
 * relinearization-key p-plane coefficient is not below P", "... a Galois-key p-plane coefficient is not below P").
 * On the device the key switch kernels are those of an ordinary set: the sum X_j is at most l N (2^w - 1) (Q P - 1) <= P5 / 2 in
 * size, so the five-prime CRT recovers it, and the epilogues of the five calls (k_eval_epilogue<true>, k_pack_finish<true>) divide
 * its magnitude by 2P limb by limb where the ordinary ones reduce it mod Q.
 * Security: the keys are RLWE samples modulo Q P, so the lattice security of a hybrid key set is that of log2(Q P) at degree N, not
 * of log2 Q.
 * Out of scope: hybrid keys for the calls that take key rows as host arrays (they always switch the ordinary way), for the hoisted
 * rotations, linear transforms, BSGS and plans (there the division by P belongs after the diagonal sum), the two-round collective
 * relinearization key modulo Q P, and a P of more than one word. */
int zkfhe_bfv_hybrid_max_p(const zkfhe_bfv_params *params, int base_bits, uint64_t *p_max);
int zkfhe_bfv_relin_keygen_hybrid(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, const uint64_t *sk, const uint8_t seed[32],
                                  int base_bits, uint64_t *rlk0_q, uint64_t *rlk1_q, uint64_t *rlk0_p, uint64_t *rlk1_p);
int zkfhe_bfv_galois_share_hybrid(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, const uint64_t *sk_i,
                                  const uint8_t crs_seed[32], const uint8_t party_seed[32], uint64_t g, int base_bits, uint64_t *r_q,
                                  uint64_t *a_q, uint64_t *r_p, uint64_t *a_p);
int zkfhe_bfv_galois_keygen_hybrid(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, const uint64_t *sk, const uint8_t seed[32],
                                   uint64_t g, int base_bits, uint64_t *gk0_q, uint64_t *gk1_q, uint64_t *gk0_p, uint64_t *gk1_p);
int zkfhe_bfv_evk_create_hybrid(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, uint64_t p, int base_bits, const uint64_t *rlk0_q,
                                const uint64_t *rlk1_q, const uint64_t *rlk0_p, const uint64_t *rlk1_p, size_t n_galois, const uint64_t *g,
                                const uint64_t *gk0_q, const uint64_t *gk1_q, const uint64_t *gk0_p, const uint64_t *gk1_p,
                                zkfhe_bfv_evk **out);
int zkfhe_bfv_evk_special_modulus(const zkfhe_bfv_evk *evk, uint64_t *p);

/* ---- Ring packing: chosen coefficients of many ciphertexts in one (bfv_pack.hip, bfv_resident.hip) ----
 * Moves one coefficient of each of n ciphertexts into one ciphertext and erases everything else (PackLWEs followed by the field
 * trace; Chen, Dai, Kim, Song 2021).  It uses Galois key switches, additions and products by a monomial only: no multiplicative
 * depth, only key-switch noise, any T (no batching modulus is needed: this is coefficient encoding), and the Galois keys of
 * zkfhe_bfv_galois_keygen or the collective keys of zkfhe_bfv_galois_share, unchanged.  Conventions of "BFV slots and rotations":
 * N uint64_t per polynomial in CircuitInput order, residues in [0, Q), "coefficient i" is the coefficient of x^i.  No new
 * randomness and no new ChaCha20 domain.  Two primitives are new:
 *   Monomial product.  x^k c mod (x^N + 1, Q) for 0 <= k < 2N: coefficient i moves to j = i + k mod 2N; for j >= N it is negated
 *     mod Q and placed at j - N.  It applies to both components and adds no noise.  For k < N it is bit for bit
 *     zkfhe_bfv_mul_plain by the plaintext x^k, for k >= N bit for bit zkfhe_bfv_mul_plain by -x^(k - N).
 *   Scaling.  Every coefficient v becomes v nu mod Q with nu = N^-1 mod Q.  Q must be odd.
 * Pack elements: g_l = 2^l + 1 for l = 1 ... log2(N), that is 3, 5, 9, ..., N + 1 (zkfhe_bfv_pack_elements; host only, g may be
 * NULL, *count = log2(N), defined for any T).  Every call uses the keys of all log2(N) of them.
 * pack of n ciphertexts a_0 ... a_(n-1) with positions pos_i < N, 1 <= n <= N, n' the least power of two >= n, L = log2(n'):
 *   1. Prepare.  w_i = nu x^((2N - pos_i) mod 2N) a_i for i < n; w_i = (0, 0) for n <= i < n'.
 *   2. Pack levels l = 1 ... L.  With h = n' / 2^l, s = N / 2^l, g = 2^l + 1, for every i < h: t = x^s w_(i+h);
 *      w_i <- (w_i + t) + zkfhe_bfv_apply_galois(w_i - t, g).  The sums and differences are those of zkfhe_bfv_add, the key switch
 *      is exactly the definition of zkfhe_bfv_apply_galois: digits of sigma_g(c1) in [0, Q).
 *   3. Trace levels l = L + 1 ... log2(N).  w_0 <- w_0 + zkfhe_bfv_apply_galois(w_0, 2^l + 1).
 *   4. The result is w_0.
 * Under the key's secret it decrypts to the plaintext whose coefficient i N / n' is coefficient pos_i of the plaintext of a_i, for
 * i < n; every other coefficient is 0.  The definition is exact, so every implementation is held to it bit for bit.
 * zkfhe_bfv_mul_monomial: host arrays, n ciphertexts; k_count is 1 (one k for all) or n; every k is below 2N.
 * zkfhe_bfv_pack: c0, c1 are [n_groups][n][N]; pos is [n_groups][n] or NULL (all 0); gk0, gk1 are [log2 N][l][N], the keys of
 * the pack elements in order (l = zkfhe_bfv_relin_digits), checked and transformed once per call; out0, out1 are [n_groups][N].
 * zkfhe_bfv_cts_mul_monomial and zkfhe_bfv_cts_pack are the same calls on resident batches, with the conventions of "Resident
 * ciphertext batches": dst of mul_monomial holds a's count and may be a; n_groups of pack is dst's count, a holds n_groups n
 * ciphertexts in [group][input] order, the keys come from the key set, dst must not be a source, nothing is allocated on the
 * device, and a refused call leaves dst as it was.
 * Refusals: ZKFHE_EINVAL with a message "bfv_pack: ...", "bfv_mul_monomial: ...", "bfv_cts_pack: ..." or "bfv_cts_mul_monomial:
 * ...", in this order and before any device work on ciphertexts: a NULL argument, a zero count or bad parameters; "Q must be odd"
 * (pack only); base_bits outside [1, 32]; "n = ... is above N"; a k_count neither 1 nor n, or a k >= 2N; a position >= N; for
 * the batch calls the device, parameter and count refusals with the texts of the other bfv_cts_* calls ("a holds H ciphertexts and
 * the call needs W", "dst must not be a source"); "the key set has no key for the Galois element G", naming the first missing
 * pack element; the coefficient >= Q checks of the host-array calls, for ciphertexts and keys.
 * Kernels.  One launch prepares every input (k_pack_prepare).  A level is a key switch that reads the digits of
 * sigma_g(e1 - x^s o1) straight from the two operands (k_key_switch: one workgroup per (pair, prime) walking the digits; or, where
 * the key is resident, l >= 2 and the level has at most zkfhe_bfv_evk_wide_max pairs, k_key_switch_digit per (digit, pair, prime)
 * followed by k_key_switch_fold) and k_pack_finish: Garner over the five primes, mod Q, plus (e0 + x^s o0) + sigma_g(e0 - x^s o0)
 * on component 0 and e1 + x^s o1 on component 1, out of place between two work arrays.  A call of more leaves than a chunk holds
 * (2^21 / N ciphertexts) reduces the subtrees of leaves with equal index mod n' / C one after another and merges their roots
 * depth first; everything is exact, so the result does not depend on the chunking.
 * Noise.  The input noise is not amplified (nu N = 1 mod Q: the N-fold sum of the trace undoes the scaling).  The key switch of
 * level l is amplified by 2^(log2 N - l).  Sufficient bound, with l_digits rows of width w and B the error bound:
 *   noise(out) <= max_i noise(a_i) + (N - 1) l_digits N (2^w - 1) B.
 * The bound is loose: at N = 1024 it certifies nothing at a 29-bit Q (2.4e9 at w = 4).  Measured (zkfhe_bfv_noise of packed fresh
 * encryptions, profiles/bfv_pack.md) at N = 1024, Q = 536870909, T = 7, where floor(Q/T)/2 = 3.8e7: a full pack of n = 1024 came to
 * 3.8e6 at w = 4 and to 3.6e7 at w = 8 (n = 1: 1.1e6 and 1.6e7).  Keep w small for packing: at these parameters w = 4 leaves a factor
 * of ten, w = 8 none.  At N = 4096, a 60-bit Q and T = 65537 (limit 8.8e12) n = 4096 came to 4.6e8 at w = 8 and 9.9e10 at w = 16. */
int zkfhe_bfv_pack_elements(const zkfhe_bfv_params *params, uint64_t *g, size_t *count);
int zkfhe_bfv_mul_monomial(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n, const uint64_t *c0, const uint64_t *c1, size_t k_count,
                           const uint64_t *k, uint64_t *out0, uint64_t *out1);
int zkfhe_bfv_pack(zkfhe_ctx *ctx, const zkfhe_bfv_params *params, size_t n_groups, size_t n, const uint64_t *c0, const uint64_t *c1,
                   const uint64_t *pos, const uint64_t *gk0, const uint64_t *gk1, int base_bits, uint64_t *out0, uint64_t *out1);
int zkfhe_bfv_cts_mul_monomial(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t k_count, const uint64_t *k, zkfhe_bfv_cts *dst);
int zkfhe_bfv_cts_pack(zkfhe_ctx *ctx, const zkfhe_bfv_cts *a, size_t n, const uint64_t *pos, const zkfhe_bfv_evk *evk, zkfhe_bfv_cts *dst);
/* zkfhe_prof_read slot of the packing kernels: algorithmic bytes = the words read and written.  k_key_switch_fold counts in
 * ZKFHE_PROF_BFV_KEY_SWITCH_WIDE; the one key transform of the host-array call in ZKFHE_PROF_RNS_NTT */
#define ZKFHE_PROF_BFV_PACK 27   /* k_pack_prepare, k_key_switch and k_key_switch_digit of a level, k_pack_finish, k_pack_monomial */

const char *zkfhe_version(void);

#ifdef __cplusplus
}
#endif
#endif
