/*
 * np_hip_debug.h — the probe side of libnp_hip.so: what tests/, tools/ and bench.py use to FORCE a kernel variant, to look
 * at a planner decision, to exercise the rendezvous / transport without peers, or to inject an error.  A binding of the
 * back end includes np_hip.h only and never calls anything declared here.
 *
 * PROCESS-GLOBAL STATE.  Every np_*_set_variant below flips a process-wide switch that stays flipped until it is set back
 * (0 / the documented "default" value): all threads and all devices of the process see it, none of them is thread-safe
 * against a concurrent launch, and a test that sets one restores it in a `finally`.  Results stay inside the documented
 * bounds under every variant — they select among kernels that compute the same thing — but bit patterns of reductions
 * and GEMMs may differ between variants (different summation order).  The np_*_debug_* / np_debug_* functions keep no
 * state except np_comm_debug_loopback (on until switched off) and np_debug_raise_device_error (raises the current
 * device's error word, which stays up until np_clear_device_error()).
 */
#ifndef NUMPOWER_AMD_NP_HIP_DEBUG_H
#define NUMPOWER_AMD_NP_HIP_DEBUG_H

#include "np_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How the communicator orders its two streams and issues the sharded GEMM (tuning / A-B; np_comm.hip):
 *   0  default: device-side flags (a one-lane kernel publishes a sequence number on the producing stream, a one-lane
 *      kernel on the consuming stream waits for it).  On a one-rank communicator the slab is ONE progress-reporting
 *      GEMM launch (piece c's transfer is released by the GEMM's own tile counter); with peers it is one GEMM launch
 *      per piece, a kernel boundary behind every piece — the single launch has only ever run on one GPU, so with
 *      world > 1 it is opt-in (3).  Falls back to HIP events by itself if the self-test at np_comm_init finds that
 *      flags do not get through (both streams on one hardware queue).
 *   1  HIP events (hipEventRecord + hipStreamWaitEvent) and one GEMM launch per piece
 *   2  device-side flags, one GEMM launch per piece
 *   3  device-side flags, ONE progress-reporting GEMM launch per slab at any world size
 * np_comm_sync_mode: 1 = flags in use, 0 = events, -1 = no communicator. */
int np_comm_set_variant(int variant);
int np_comm_sync_mode(void);

/* testing: the rendezvous of np_comm_init alone (no device, no RCCL) — rank 0's 128 bytes reach every peer */
int np_comm_debug_exchange(int rank, int world, const char *endpoint, void *bytes128, double timeout_s);
/* testing: the exchange np_sgemm_strided_batched_allgather makes rank `rank` of `world` issue for a slab of `slab` items
 * of item_bytes in `chunks` pieces (point to point), computed by the same functions as the real path, without a device or
 * a communicator: records {piece, send to, send offset, bytes, receive from, receive offset} (byte offsets into the
 * replicated result); *host_count = number of records (also when max_records is smaller). */
int np_comm_debug_plan(int rank, int world, size_t slab, size_t item_bytes, int chunks, unsigned long long *host_out,
                       size_t max_records, size_t *host_count);
/* the step model behind np_sgemm_strided_batched_allgather(chunks = 0) (np_comm.hip: model_pieces), for any
 * world / shape on a device of `cus` CUs (0 = 256), without a device or a communicator: *host_chunks = the piece count it
 * picks; host_ms5 (may be NULL) = the modelled step in ms with 1, 2, 4, 8, 16 pieces. */
int np_comm_debug_model(int world, size_t slab, size_t M, size_t N, size_t K, int cus, int *host_chunks, double *host_ms5);
/* testing: dst <- src through one grouped ncclSend / ncclRecv pair from this rank to itself on the communication
 * stream, then np_comm_wait() — the P2P transport on a box with a single GPU */
int np_comm_debug_sendrecv_self(const void *dev_src, void *dev_dst, size_t bytes);
/* testing: `count` (<= 64) self transfers of `bytes` on the communication stream, not ordered behind the library stream (so
 * they compete with whatever that stream is running), each bracketed by its own events; host_ms[i] = duration of transfer i.
 * Returns when the communication stream has drained. */
int np_comm_debug_loopback_timed(const void *dev_src, void *dev_dst, size_t bytes, int count, float *host_ms);
/* testing: every piece gathered point-to-point is from now on ALSO sent from this rank to itself into dev_scratch
 * (pieces larger than `bytes` are not): real RCCL traffic next to the GEMM on a box without a peer.  (NULL, 0) = off. */
int np_comm_debug_loopback(void *dev_scratch, size_t bytes);

/* Kernel-variant selection for tuning/benchmarks (0 = default heuristic; -1 = whole-K plans only (no split-K, no
 * stream-K), -2 = default planner again, -3 = default planner + always pad unaligned operands, -4 = stream-K wherever
 * the kernel can run it, -5 = default planner without stream-K, -6 = operands whose rows are not float4-loadable never
 * go to the LDS-DMA kernel as they are (padded copies / register-staged kernels, as before round 3), -8 = they always do, whatever the size, -7 = back to the
 * default: from a size threshold up), -9 = never peel a thin ragged edge (M % 256 <= 32 rows, N % 128 <= 2 columns) off a
 * large product, -11 = always when there is one, -10 = back to the default: when the planner's model says it pays), -12 = products with M <= 64 rows go to the tiled
 * kernels instead of sgemm_fewrows_kernel / sgemm_skinny_kernel (as before round 3), -13 = back; round 4: -14 / -15 = plans
 * without / with the mid-size LDS-DMA tiles (sgemm_dmas_kernel), -16 / -17 = their tiles walked row-major / in XCD-aware bands,
 * -18 / -19 = ragged whole-K 64 x 64 products on four / eight waves, -20 / -21 = plans without / with the k-quartered tiles
 * (sgemm_kq_kernel); -(1000 + 100 * shape + S) forces sgemm_dmas_kernel's tile `shape` with K split S ways wherever it applies,
 * -(2000 + shape) forces sgemm_kq_kernel's tile `shape` (0 .. 6: 48x48, 32x32, 64x64, 48x32, 64x32, 64x48, 80x48), -999 ends
 * either forcing; round 5, deep-K products of a few tiles: -22 / -23 = plans without / with K-chunks on the k-quartered tiles,
 * -24 = that plan wherever one exists, -25 / -26 = its launch tile-major / chunk-major over the XCDs, -(30000 + 1000 * shape + S)
 * forces single products of K >= 512 onto S K-chunks of k-quartered tile `shape` (-30000: off), -(40 + q), q = 0 .. 59: a thin
 * K-chunk launch (17 .. 2047 rows, N <= 64, K >= 16384) of fewer than q / 4 workgroups per CU goes to the planner instead
 * (0 = never, as before round 5; default 59); -27 / -28 = consecutive independent large products on the library stream alone /
 * alternating with the side stream (np_sgemm_overlap_stats, np_hip.h; default), -29 = products of any size qualify for that
 * (tests), -30 = from 4e9 flop again; -31 / -32 = the K loop of the 256 x 128 LDS-DMA kernels (sgemm_dma_kernel, sgemm_streamk_kernel)
 * with flat per-lane source pointers everywhere / with buffer-addressed sources and three K-tiles per trip wherever the launch is
 * eligible (no K % 16 / N % 4 tail, A and B 16-byte aligned, lda and ldb multiples of 4 below 2^22), -33 = the default: the second
 * form for the eligible whole-tile launches with full tiles and K >= 2048 (the instantiation measured faster beyond its noise,
 * profiles/kloop/), the first for the rest — same bits either way, np_sgemm_debug_kloop_stats counts which loop each launch ran.  All of them are process-wide setters for A/B measurements and tests: results stay within the same bounds. */
int np_runtime_set_variant(int variant);   /* how host-result calls wait: 0 = hipStreamSynchronize, 1 = spin on a stream-written flag, 2 = spin on the result itself (default) */
int np_sgemm_set_variant(int variant);
/* tests / tools: out[0] = launches of sgemm_dma_kernel / sgemm_streamk_kernel that ran the buffer-addressed K loop (-32) so far,
 * out[1] = those that ran the flat-addressed one (-31, or a launch that is not eligible) */
int np_sgemm_debug_kloop_stats(unsigned long long out[2]);
/* tests: C (M x N, rows ldc floats apart) = A (M x K, rows lda apart) . B (K x N, rows ldb apart) — one np_sgemm on windows of larger
 * buffers, the form the factorizations use internally; nothing outside the windows is read into C or written */
int np_sgemm_debug_ld(size_t M, size_t N, size_t K, const float *A, size_t lda, const float *B, size_t ldb, float *C, size_t ldc);
/* debug: the planner's choice for one dense, aligned M x N x K product on a device of `cus` CUs (0 = the current device; any
 * other value needs no device: the planner is host arithmetic).  out[11]: cfg, tail_rows, S, modelled us of the tiled plan;
 * stream-K taken (0/1), its modelled us; cfg, S, us of the best mid-size-tile plan; cfg, us of the best plan without them
 * (1e300 = does not apply).  tests/test_abi_and_host_cpu.py pins the choices that matter (no reference counterpart:
 * linalg.c:75-79 hands every product to cblas / cuBLAS). */
int np_sgemm_debug_plan(size_t M, size_t N, size_t K, size_t batch, int cus, double *out);
/* debug: the same decision for ONE dense M x N x K product whose rows are not float4-loadable (K % 4 or N % 4 != 0, or operands off
 * 16 bytes).  out[5]: cfg, tail_rows, S of the tiled plan of the product as it is; stream-K taken instead (0/1); padded copies and
 * the aligned kernel taken instead of either (0/1).  Host arithmetic, like np_sgemm_debug_plan. */
int np_sgemm_debug_plan_unaligned(size_t M, size_t N, size_t K, int cus, double *out);
/* A/B switches of single kernels of np_elementwise.hip / np_fused_chain.hip, same bits either way; a plain setter, 0 = defaults.  7000: chains on
 * the interpreter only (no compiled chain); 7001: chains that name an array twice as every other chain (compiled or streaming), 7002: never
 * looked for; 7004: compiled first-axis chains with 4 rows in flight; 8000: a long row operand in the plain work order; 8100 / 8101: the 2-D
 * broadcast kernels off / on again (kept beside the code: it does not replace it); 9000: np_binary(pow) with its log2 table in LDS instead of
 * registers; 12000 + k / 14000 + k: first-axis chains on k workgroups per CU, compiled ones with 2 / 4 rows in flight.  Any non-zero code also
 * keeps FULL (op) ROW off the 2-D form. */
int np_elementwise_set_variant(int variant);
/* A/B switches of np_layout.hip, same bits either way.  Plain codes (one value, 0 = default): 64 / 128 force the transpose tile (and keep
 * the interleave, skinny, write-aligned and plane kernels off), 1 = default tiles without the write-aligned form for output rows off
 * the 128-byte grid, 3 / 4 = np_permute without the plane path, 5 = no interleave, 6 = the plane path on single floats only, 7 =
 * write-aligned tiles of 64 always.  Separate values: 7000 + N = write-aligned transposes below N tiles of 128 take tiles of 64
 * (default 1200, 0 = never); 17000 + k = the write-aligned tile order k = 0 / 1 / 2, 17003 = by size; 17010 + k = the tile kernel's
 * order, 17013 = default; 17020 + k = the plane kernel's, 17023 = default.  Everything back: 0, 8200, 17003, 17013, 17023. */
int np_layout_set_variant(int variant);
int np_select_set_variant(int variant);   /* order statistics: 0 = plain three passes only (no bracket path, no one-workgroup kernel), 1 = default (n >= 2^26), else the smallest n that takes it */
int np_select_last_path(int *path);       /* tests / tools: 1 if the last selection ran over the bracket's copied keys, 0 if over the array, 2 if in the one-workgroup kernel (synchronises) */
int np_reduce_set_variant(int variant);   /* streaming reductions, first pass: workgroups per CU (0 = default) */
/* tools: the shader clock in MHz a ~20 us probe kernel sees on the library stream right now (synchronises the stream) */
int np_debug_clock_mhz(float *host_mhz);
/* tools: host_out2[2 w] = HW_REG_HW_ID, host_out2[2 w + 1] = HW_REG_XCC_ID of workgroup w of a `workgroups`-wide launch of one-wave
 * workgroups on the library stream (each spins ~10 us first): where a (CU-masked) stream's work lands (tools/cu_mask_probe.py) */
int np_debug_hw_ids(unsigned *host_out2, size_t workgroups);
/* tools: the CU count every planner (GEMM tiles / stream-K, streaming grids) assumes from now on; 0 = the device's own.  For a CU-masked
 * library stream (np_set_stream): a product planned for 256 CUs runs a partial extra round of workgroups on 248.  Process-global. */
int np_debug_set_cus(int cus);
/* tests: the CU count the planners assume right now (np_debug_set_cus's value, else the current device's own): what a test needs to
 * work out which kernel a shape is planned onto. */
int np_debug_cus(int *host_cus);
/* testing: a one-lane kernel on the library stream raises `bits` in the current device's error word — what a device-side wait
 * that gives up does (1 = a stream-ordering wait of np_comm, 2 = a stream-K finisher).  np_sync / np_memcpy_d2h / host-result
 * calls / np_comm_* calls on this device return NP_ERR_DEVICE from then on, until np_clear_device_error(). */
int np_debug_raise_device_error(unsigned bits);
/* testing: kernel launches the library has issued since it was loaded (all devices, all threads): the difference around an
 * expression is how many launches it cost — `nd::exp($a) * $b + 2` through the pending chains of INTEGRATION.md 2c: one. */
int np_debug_launch_count(unsigned long long *host_count);
/* testing: the sweep cap of np_svd / np_svdvals from now on (0 = the default, 60): with 1 a dense matrix cannot converge, which
 * is how a test reaches info > 0 without a pathological matrix.  Process-global. */
int np_debug_svd_max_sweeps(int sweeps);
/* tools: sweeps the last np_svd / np_svdvals call of the process took (the converged one, which rotates nothing, included).
 * A plain process global, like the two knobs around it: meaningful only while one thread calls the SVD. */
int np_debug_svd_last_sweeps(int *host_sweeps);
/* testing / A-B: on = 0 sends every shape through the blocked path, on != 0 (the default) lets min(m, n) <= 64 with a row
 * length that fits LDS take the one-launch kernel.  Process-global. */
int np_debug_svd_small_path(int on);
/* the same three for np_eigh / np_eigvalsh: the sweep cap (0 = the default, 60), the sweeps the last call took (the converged
 * one, which rotates nothing, included), and on = 0 sending n <= 64 through the blocked path too.  Process-global. */
int np_debug_eigh_max_sweeps(int sweeps);
int np_debug_eigh_last_sweeps(int *host_sweeps);
int np_debug_eigh_small_path(int on);
/* tests / tools: the path the last np_correlate2d call of the process took: 1 = staged once (window up to 15 x 15), 2 = chunked,
 * 0 = none yet.  A plain process global. */
int np_debug_conv2d_last_path(int *host_path);
/* testing / A-B: on = 0 sends every window through the chunked path, on != 0 (the default) lets windows up to 15 x 15 be staged
 * once.  Process-global. */
int np_debug_conv2d_staged_path(int on);
/* tests / tools: what the last np_conv2d_forward / _backward_data / _backward_filter call of the process launched: the tile's row
 * count TM (32, 64 or 128; 0 = none yet) and, for _backward_filter, the number of slices S its reduction was cut into (1: written
 * directly, no fold kernel); 0 slices after the two others.  Plain process globals. */
int np_debug_dnn_last_path(int *host_tm, int *host_slices);
/* tests / tools: the form of the gather that call compiled to: 0 unit (stride 1, dilation 1), 1 strided / dilated window,
 * 2 dilated input (the data gradient of a strided layer). */
int np_debug_dnn_last_form(int *host_form);
/* tests / tools: the epilogue of the last forward launch of the process (np_conv_act and whether a bias was added; 0, 0 for the
 * plain kernels, the data gradient included) and the number of slices S of the last np_conv2d_backward_act call that produced
 * a db (1: written directly, no fold kernel).  (0, 0, 0) before any launch. */
int np_debug_dnn_last_epilogue(int *act, int *has_bias, int *bias_slices);
/* tests / tools: the kernel forms the last np_pool2d_forward and the last np_pool2d_backward of the process launched: forward
 * 1 = direct (one lane per output, planes of more than 8192 cells), 2 = staged (whole planes through LDS, H.W <= 8192);
 * backward 1 = gather (one lane per dx cell).  (0, 0) before any launch; NP_ERR_INVALID on a null pointer.  Plain process globals. */
int np_debug_pool_last_path(int *forward_form, int *backward_form);
/* testing / A-B: form = 1 sends every shape through the direct forward form, form = 0 (the default) chooses by the extents.
 * The two forms return the same bits.  Process-global. */
int np_debug_pool_forward_form(int form);
/* tests / tools: the kernel form the last np_softmax_forward, np_softmax_backward or np_cross_entropy of the process launched:
 * 1 = short rows (slabs of whole rows through LDS), 2 = a wave per row, 3 = a workgroup per row, 4 = streaming (two reads),
 * 5 = strided (inner > 1, a lane per column).  0 before any launch; NP_ERR_INVALID on a null pointer.  A plain process global. */
int np_debug_softmax_last_path(int *form);
/* testing / A-B: form = 1 .. 5 sends every call through that form, -1 (the default) chooses by (cols, inner).  A call whose shape
 * the forced form cannot serve is refused (NP_ERR_INVALID) before any device work.  Process-global. */
int np_debug_softmax_force_form(int form);
/* the boundaries, n >= 5: bounds[0 .. 2] = the largest cols of the short, wave and workgroup forms, bounds[3] = the words of
 * one staged slab, bounds[4] = the most rows a slab holds (rows per slab = min(bounds[4], bounds[3] / (cols | 1))) */
int np_debug_softmax_bounds(size_t bounds[], int n);
/* tests / tools: what the last np_batchnorm_forward or np_batchnorm_backward of the process launched.  form: 1 = one launch, a
 * workgroup per channel with the channel in registers, 2 = split (statistics per (channel, slice), fold, apply), 3 = rows
 * (inner == 1: lanes along C, slices of N), 4 = inference (the apply kernel alone).  launches: the kernels it took (1 for forms 1
 * and 4, 3 for forms 2 and 3).  slices: S of forms 2, 3 and 4, 0 for form 1.  Zeros before any launch; NP_ERR_INVALID on a null
 * pointer.  Plain process globals. */
int np_debug_batchnorm_last_path(int *form, int *launches, size_t *slices);
/* testing / A-B: form = 1 .. 3 sends every call through that form (inference: through that form's apply kernel; 1 counts as 2
 * there), -1 (the default) chooses by (N, inner).  A call whose shape the forced form cannot serve is refused (NP_ERR_INVALID)
 * before any device work.  Process-global. */
int np_debug_batchnorm_force_form(int form);
/* the boundaries, n >= 5: bounds[0] = the most values of a channel that form 1 takes on 256 lanes, bounds[1] = on 1024 lanes (the
 * largest n of form 1), bounds[2] = the workgroups the slices aim for, bounds[3] = the most slices, bounds[4] = the fewest
 * workgroup steps a slice holds */
int np_debug_batchnorm_bounds(size_t bounds[], int n);
/* tests / tools: what the last np_groupnorm_forward or np_groupnorm_backward of the process launched.  row_form: 1 = short rows
 * (a power-of-two segment of a wave per row), 2 = a wave per row, 3 = a workgroup per row (both with the row in registers),
 * 4 = split (statistics per (row, slice), fold, apply).  param_form: 0 = no parameter reduction (the forward pass; dgamma and
 * dbeta both NULL), 1 = columns (inner == 1), 2 = planes.  launches: the kernels it took (1 or 3 for the rows, 2 for the
 * parameters).  row_slices: S of row form 4, 0 otherwise.  param_slices: the slices of the parameter reduction, 0 without one.
 * Zeros before any launch; NP_ERR_INVALID on a null pointer.  Plain process globals. */
int np_debug_groupnorm_last_path(int *row_form, int *param_form, int *launches, size_t *row_slices, size_t *param_slices);
/* testing / A-B: row_form = 1 .. 4 and param_form = 1 .. 2 send every call through that form, -1 (the default) chooses by
 * (D, inner).  A call whose shape a forced form cannot serve is refused (NP_ERR_INVALID) before any device work.  Process-global. */
int np_debug_groupnorm_force_form(int row_form, int param_form);
/* the boundaries, n >= 7: bounds[0 .. 1] = the largest L of the short and the wave form, bounds[2] = the largest L a workgroup
 * of 256 lanes takes, bounds[3] = of 1024 lanes (the largest L of form 3), bounds[4] = the workgroups the slices aim for,
 * bounds[5] = the most slices, bounds[6] = the fewest workgroup steps a slice holds */
int np_debug_groupnorm_bounds(size_t bounds[], int n);
/* tests / tools: what the last np_attention_forward or np_attention_backward of the process launched.  d_class: the D
 * instantiation (32, 64 or 128).  q_tile, k_tile: the query rows of a workgroup and the keys of a staged tile.  launches: the
 * kernels it took (1 forward; backward 1 for delta, 1 for dk / dv unless both are NULL, 1 for dq unless it is NULL, 0 with all
 * three NULL).  key_tiles: the key tiles the workgroup of the LAST query rows visits.  skipped: the (query workgroup, key tile)
 * pairs of one slice that causal skips, 0 without causal.  Zeros before any launch; NP_ERR_INVALID on a null pointer.  Plain
 * process globals. */
int np_debug_attention_last_path(int *d_class, int *q_tile, int *k_tile, int *launches, size_t *key_tiles, size_t *skipped);
/* the constants, n >= 7: bounds[0] = the query rows of a workgroup, bounds[1] = the keys of a staged tile (T of the causal
 * rule), bounds[2 .. 4] = the largest D of the three instantiations, bounds[5] = the rows of a wave, bounds[6] = the keys of a
 * workgroup of the dk / dv kernel */
int np_debug_attention_bounds(size_t bounds[], int n);
/* tests / tools: what the last np_sgd_step, np_adam_step or np_grad_norm of the process launched.  launches: the kernels it took
 * (a step: ceil(T / bounds[1]); the norm: that many and the fold).  chunks: the chunks of all its launches (a step: per tensor
 * ceil((o + n) / bounds[0]) with o = (the pointers' common residue mod 16) / 4 for a tensor served with 16-byte accesses and
 * o = 0 for a scalar one; the norm: per tensor ceil(n / bounds[2]), one partial each).  vec_tensors, scalar_tensors: the tensors of
 * a step by access form (both 0 for the norm).  Zeros before any launch; NP_ERR_INVALID on a null pointer.  Plain process globals. */
int np_debug_optim_last_path(int *launches, size_t *chunks, int *vec_tensors, int *scalar_tensors);
/* the constants, n >= 5: bounds[0] = the elements of a step chunk, bounds[1] = kOptimMaxTensors, the tensors of one launch,
 * bounds[2] = the elements behind one partial of np_grad_norm (its slice rule: tensor t gives ceil(n_t / bounds[2]) partials, in
 * list order), bounds[3] = the workgroups per CU that cap a grid (min(chunks, CUs . bounds[3] | 1)), bounds[4] = the bytes of
 * the list as a kernel argument */
int np_debug_optim_bounds(size_t bounds[], int n);
/* testing / A-B: on != 0 serves every tensor of a step with scalar accesses, 0 (the default) chooses per tensor by the pointers'
 * residues.  Both forms give the same bits.  Process-global. */
int np_debug_optim_force_scalar(int on);
/* tests / tools: what the last np_linear_forward (product 0) or np_linear_backward (products 1 .. 3) of the process launched for
 * one product: 0 = y, 1 = dx, 2 = dw, 3 = the dz / db kernel.  form: 1 = the tile form, 2 = the library form over np_sgemm (0: the last
 * call did not launch this product; product 3 always reports 1).  tm: the tile's row count (32, 64 or 128; 0 for product 3 and for
 * the library form).  slices: S of dw, S' of dz / db, 1 for y and dx; 0 for the library form.  launches: the kernels the product took
 * (tile form: 1, or 2 with a fold; library form: the transpose, np_sgemm's own launches and the bias / activation pass).  A backward call clears products 1 .. 3 first, so a product that
 * was not asked for reads (0, 0, 0, 0).  NP_ERR_INVALID on a null pointer or an unknown product.  Plain process globals. */
int np_debug_linear_last_path(int product, int *form, int *tm, int *slices, int *launches);
/* testing / A-B: form = 1 sends every product through the tile form, 2 through the library form, 0 (the default) chooses per
 * product by (M, K, N).  NP_ERR_INVALID for any other value.  Process-global. */
int np_debug_linear_force_form(int form);
/* the constants, n >= 16: bounds[0 .. 2] = the three TM, bounds[3] = the tile's columns, bounds[4] = the reduction step,
 * bounds[5 .. 7] = dw's slice rule (the fewest steps of a slice, the workgroups the slices aim for, the most slices),
 * bounds[8 .. 12] = the dz / db kernel (the columns of a workgroup, its row groups, the fewest rows of a slice, the workgroups the
 * slices aim for, the most slices), bounds[13 .. 15] = the multiply-adds M.K.N from which y, dx and dw take the library form */
int np_debug_linear_bounds(size_t bounds[], int n);
/* tests / tools: which kernel families the last np_reduce_axis or np_reduce_all(_dev) call of the process launched, the calls it
 * makes on its own partials included: the OR of the NP_REDUCE_PATH_ bits below (0 = none yet).  A plain process global, cleared
 * at the top of those entry points; calls the library makes itself (split-K GEMM folds, chain partials) overwrite it too. */
#define NP_REDUCE_PATH_ROWS_BLOCK 0x0001u          /* inner == 1: reduce_rows_block, a workgroup per row */
#define NP_REDUCE_PATH_ROWS_BLOCK_CHUNKED 0x0002u  /* reduce_rows_block over chunks of each row; the partials are reduced again */
#define NP_REDUCE_PATH_ROWS_STAGED 0x0004u         /* reduce_rows_staged: slabs of short rows through LDS */
#define NP_REDUCE_PATH_ROWS_GROUP 0x0008u          /* reduce_rows_group<L>: L = 2 .. 32 lanes per row */
#define NP_REDUCE_PATH_ROWS_WAVE 0x0010u           /* reduce_rows_wave: a wave per row */
#define NP_REDUCE_PATH_COLS_ONE_PASS 0x0020u       /* inner > 1: reduce_axis_cols writes the result */
#define NP_REDUCE_PATH_COLS_TWO_PASSES 0x0040u     /* reduce_axis_cols over 2 .. 255 splits of the axis + reduce_axis_cols over the partials */
#define NP_REDUCE_PATH_COLS_SPLITS_RECURSE 0x0080u /* reduce_axis_cols over >= 256 splits; the partials are reduced again */
#define NP_REDUCE_PATH_COLS_XCD_RUNS 0x0100u       /* a reduce_axis_cols launch dealt its tiles to the XCDs in runs */
#define NP_REDUCE_PATH_SMALL_INNER 0x0200u         /* reduce_small_inner (dword walk); the partials are reduced again */
#define NP_REDUCE_PATH_SMALL_INNER_V4 0x0400u      /* reduce_small_inner_v4 (float4 walk); the partials are reduced again */
#define NP_REDUCE_PATH_GENERIC 0x0800u             /* reduce_axis_generic, a thread per output */
#define NP_REDUCE_PATH_GENERIC_CHUNKED 0x1000u     /* reduce_axis_generic over chunks of the axis; the partials are reduced again */
#define NP_REDUCE_PATH_ALL_ONE_LAUNCH 0x2000u      /* reduce_all_pass1, folded by its last workgroup */
#define NP_REDUCE_PATH_ALL_TWO_LAUNCHES 0x4000u    /* reduce_all_pass1 + reduce_all_pass2 */
int np_debug_reduce_last_path(unsigned *host_mask);
/* the same for the last np_fused_chain_reduce / _reduce_dev / _reduce_axis call: the OR of the NP_CHAIN_PATH_ bits.  Partials
 * (NP_CHAIN_PATH_SPLIT) and the temporary go through np_reduce_axis, whose own probe then tells how. */
#define NP_CHAIN_PATH_FLAT 0x0001u         /* full reduction: fused_chain_kernel (the interpreter) */
#define NP_CHAIN_PATH_STATIC_FLAT 0x0002u  /* full reduction: a compiled chain (np_fused_static.hip) */
#define NP_CHAIN_PATH_ROWS 0x0004u         /* last axis: fused_chain_rows_kernel */
#define NP_CHAIN_PATH_ROWS_STAGED 0x0008u  /* last axis: fused_chain_rows_staged_kernel */
#define NP_CHAIN_PATH_STATIC_ROWS 0x0010u  /* last axis: a compiled chain */
#define NP_CHAIN_PATH_COLS 0x0020u         /* first axis: fused_chain_cols_kernel */
#define NP_CHAIN_PATH_STATIC_COLS 0x0040u  /* first axis: a compiled chain */
#define NP_CHAIN_PATH_SPLIT 0x0080u        /* the axis was cut into chunks: np_reduce_axis folds the partials */
#define NP_CHAIN_PATH_TEMPORARY 0x0100u    /* the chain was stored to a temporary and np_reduce_axis reduced it */
int np_debug_chain_reduce_last_path(unsigned *host_mask);
/* the same for the product kernels of np_sgemm.hip: the OR of the NP_SGEMM_PATH_ bits naming everything the last np_sgemm /
 * np_sgemm_strided_batched / np_sgemm_debug_ld / np_sgemv call of the process launched (0 = none yet).  A plain process global,
 * cleared at the top of the OUTERMOST of those entry points only: the calls they make among themselves (N = 1 of a thin product
 * is np_sgemv, a peeled product hands its edges to np_sgemm_strided_batched) OR into the mask of the call that made them.  Bits
 * 0 .. 19 name kernels; the two fields above them carry the template argument where it selects another instantiation: bits
 * 20 .. 23 = log2(L) + 1 of the lane-group width L of sgemm_thin_kernel / sgemv_short_rows_kernel, bits 24 .. 27 = log2(MV) + 1
 * of the accumulator count MV of sgemm_fewrows_kernel / sgemm_thin_left_kernel (0 = no such kernel ran).  NP_SGEMM_PATH_LANES(L)
 * and NP_SGEMM_PATH_MV(MV) build the fields, so a test writes a whole mask: NP_SGEMM_PATH_THIN_LANES | NP_SGEMM_PATH_LANES(8).
 * Costs one store to a host global per launch site: no device work, no synchronisation.  Like the probes above it is meaningful
 * only while one thread calls the products. */
#define NP_SGEMM_PATH_THIN_LANES 0x00001u          /* sgemm_thin_kernel<NV, L>; L in the LANES field */
#define NP_SGEMM_PATH_THIN_MFMA16 0x00002u         /* sgemm_thin_mfma_kernel<16> (N <= 16) */
#define NP_SGEMM_PATH_THIN_MFMA32 0x00004u         /* sgemm_thin_mfma_kernel<32> (N <= 32) */
#define NP_SGEMM_PATH_THIN_MFMA32X2 0x00008u       /* sgemm_thin_mfma_kernel<32, 2> (N = 33 .. 64) */
#define NP_SGEMM_PATH_THIN_K_CHUNKS 0x00010u       /* that launch had gridDim.y > 1: K-chunks into partials */
#define NP_SGEMM_PATH_FEWROWS_SPLITK1 0x00020u     /* sgemm_fewrows_splitk_kernel<1> (N <= 32) */
#define NP_SGEMM_PATH_FEWROWS_SPLITK2 0x00040u     /* sgemm_fewrows_splitk_kernel<2> (N = 33 .. 64) */
#define NP_SGEMM_PATH_THIN_CHUNKS 0x00080u         /* sgemm_thin_chunks_kernel<NV> */
#define NP_SGEMM_PATH_FEWROWS 0x00100u             /* sgemm_fewrows_kernel<MV>; MV in the MV field */
#define NP_SGEMM_PATH_SKINNY 0x00200u              /* sgemm_skinny_kernel */
#define NP_SGEMM_PATH_FOLD 0x00400u                /* a launcher folded its partials with np_reduce_axis */
#define NP_SGEMM_PATH_THIN_LEFT 0x00800u           /* sgemm_thin_left_kernel<MV>; MV in the MV field */
#define NP_SGEMM_PATH_PEELED 0x01000u              /* try_peeled took the shape: main block + edge products */
#define NP_SGEMM_PATH_GEMV_STAGED 0x02000u         /* sgemv_staged_rows_kernel */
#define NP_SGEMM_PATH_GEMV_SHORT_ROWS 0x04000u     /* sgemv_short_rows_kernel<L>; L in the LANES field */
#define NP_SGEMM_PATH_GEMV_FEWROWS_CHUNKS 0x08000u /* sgemv_fewrows_chunks_kernel */
#define NP_SGEMM_PATH_GEMV_CHUNKS 0x10000u         /* sgemv_chunks_kernel */
#define NP_SGEMM_PATH_GEMV_WAVE 0x20000u           /* sgemv_kernel, a wave per row */
#define NP_SGEMM_PATH_GEMV_WAVE_VEC 0x40000u       /* ... in its aligned float4 form (vec) */
#define NP_SGEMM_PATH_TILED 0x80000u               /* launch_sgemm reached: the planner's tiled, stream-K, padded, mid or kq plans */
#define NP_SGEMM_PATH_LANES(L) ((unsigned)(__builtin_ctz((unsigned)(L)) + 1) << 20)   /* L = 1, 2, 4 .. 64 */
#define NP_SGEMM_PATH_MV(MV) ((unsigned)(__builtin_ctz((unsigned)(MV)) + 1) << 24)    /* MV = 1, 2, 4, 8, 16 */
int np_sgemm_debug_last_path(unsigned *host_mask);
/* Everything behind NP_SGEMM_PATH_TILED, launch by launch: one record of NP_SGEMM_LAUNCH_WORDS unsigned words per kernel launch
 * the last outermost product call (the entry points above, and np_sgemm_debug_sub_ld) made behind launch_sgemm_ld, in launch
 * order, cleared where the mask is cleared.  The first NP_SGEMM_LAUNCH_KEPT launches are kept; *host_count is the number of
 * launches made, exact also when it is larger than that or than `capacity` (records).  min(count, kept, capacity) records are
 * written.  The fold of a split-K plan is np_reduce_axis's launch and shows as NP_SGEMM_PATH_FOLD in the mask, not here.  Host
 * stores at the launch sites, like the mask: no device work, no synchronisation; one thread at a time.  A record:
 *   word 0  NP_SGEMM_LAUNCH_FAMILY: the kernel
 *   word 1  NP_SGEMM_LAUNCH_TILE: bm | bn << 16, the tile of C one workgroup owns (0 for pad_copy_kernel)
 *   word 2  NP_SGEMM_LAUNCH_BK: the K-tile depth bk | (shape + 1) << 16, shape = the index np_sgemm_set_variant names for
 *           sgemm_dmas_kernel (0 .. 5: the instantiated DmasShape, 5 = 64 x 64 on eight waves) and sgemm_kq_kernel (0 .. 6); 0 in
 *           the high half for the kernels without one
 *   word 3  NP_SGEMM_LAUNCH_FLAGS: the template arguments and launch forms, NP_SGEMM_LAUNCH_F_ bits
 *   word 4  NP_SGEMM_LAUNCH_S: sgemm_dmas_kernel: the S K-chunks per tile after the launcher's clamp; sgemm_kq_kernel launched
 *           chunk-major: GemmArgs::k_chunks, the K-chunks inside grid.x; pad_copy_kernel: the row length of the padded copy; else 1
 *           (the K-chunks of a split-K plan run as the batch: grid.z)
 *   word 5  NP_SGEMM_LAUNCH_GRID_X, word 6 NP_SGEMM_LAUNCH_GRID_Z: gridDim.x and gridDim.z (gridDim.y is 1 everywhere)
 *   word 7  NP_SGEMM_LAUNCH_K_LAST: the length of the remainder chunk that rides as the last batch entry (0 = none) */
#define NP_SGEMM_LAUNCH_WORDS 8u
#define NP_SGEMM_LAUNCH_KEPT 16u
#define NP_SGEMM_LAUNCH_FAMILY 0
#define NP_SGEMM_LAUNCH_TILE 1
#define NP_SGEMM_LAUNCH_BK 2
#define NP_SGEMM_LAUNCH_FLAGS 3
#define NP_SGEMM_LAUNCH_S 4
#define NP_SGEMM_LAUNCH_GRID_X 5
#define NP_SGEMM_LAUNCH_GRID_Z 6
#define NP_SGEMM_LAUNCH_K_LAST 7
#define NP_SGEMM_KERNEL_TILE 1u      /* sgemm_kernel<BM, BN, BK, MINW, VEC, EDGE> (the register-staged tiles) */
#define NP_SGEMM_KERNEL_PIPE 2u      /* sgemm_pipe_kernel<128, 128, VEC, EDGE, MODE>; NP_SGEMM_LAUNCH_F_PIPE_MODE1 for MODE = 1 */
#define NP_SGEMM_KERNEL_DMA 3u       /* sgemm_dma_kernel<EDGE, KTAIL, PRIO, BUF> (256 x 128) */
#define NP_SGEMM_KERNEL_STREAMK 4u   /* sgemm_streamk_kernel<EDGE, KTAIL, PRIO, BUF>; grid.x = the G workgroups */
#define NP_SGEMM_KERNEL_DMAS 5u      /* sgemm_dmas_kernel<DmasShape, EDGE, KTAIL> */
#define NP_SGEMM_KERNEL_KQ 6u        /* sgemm_kq_kernel<TM, TN, STAGES, EDGE, VEC> */
#define NP_SGEMM_KERNEL_PAD_COPY 7u  /* pad_copy_kernel */
#define NP_SGEMM_KERNEL_TILE_SUB 8u  /* sgemm_kernel<128, 128, 16, 2, VEC, EDGE, SUB = true> (np::sgemm_sub_ld) */
#define NP_SGEMM_LAUNCH_F_VEC 0x001u          /* float4 loads of A and B */
#define NP_SGEMM_LAUNCH_F_EDGE 0x002u         /* the guarded M / N (register-staged tiles: and K) edges */
#define NP_SGEMM_LAUNCH_F_KTAIL 0x004u        /* the last K-tile's fix-up */
#define NP_SGEMM_LAUNCH_F_PRIO 0x008u         /* priority alternation */
#define NP_SGEMM_LAUNCH_F_BUF 0x010u          /* the buffer-addressed K loop */
#define NP_SGEMM_LAUNCH_F_SUB 0x020u          /* C -= A . B */
#define NP_SGEMM_LAUNCH_F_SWIZZLE 0x040u      /* GemmArgs::swizzle != 0: tiles walked in XCD-aware bands */
#define NP_SGEMM_LAUNCH_F_CHUNK_MAJOR 0x080u  /* sgemm_kq_kernel: GemmArgs::k_chunks != 0, the K-chunks folded into grid.x */
#define NP_SGEMM_LAUNCH_F_PIPE_MODE1 0x100u   /* sgemm_pipe_kernel<.., MODE = 1> */
int np_sgemm_debug_last_launches(unsigned *host_records, unsigned capacity, unsigned *host_count);
/* tests: C (M x N, rows ldc apart) -= A (M x K, rows lda apart) . B (K x N, rows ldb apart) — np::sgemm_sub_ld, the trailing update of
 * the LU and the Cholesky, on its own: one launch of the subtracting 128 x 128 tile kernel on the library stream.  Checked like
 * np_sgemm_debug_ld; clears and fills the two probes above like a product call (the mask reads 0: no np_sgemm path ran). */
int np_sgemm_debug_sub_ld(size_t M, size_t N, size_t K, const float *A, size_t lda, const float *B, size_t ldb, float *C, size_t ldc);
/* tests / tools: what the last np_transpose2d, np_permute, np_strided_copy or np_copy2d call of the process launched: ONE record of
 * NP_LAYOUT_RECORD_WORDS unsigned words for the kernel (or device copy) that finally ran.  Cleared at the top of each of those entry
 * points, so np_permute handing its fused shape to np_transpose2d leaves the record of the transpose kernel alone; *host_count = the
 * launches noted since the record was cleared (0: none yet, or a call that had nothing to move; else 1).  `capacity` counts records:
 * min(count, capacity) records are written.  Host stores at the launch sites: no device work, no synchronisation; plain process
 * globals, meaningful only while one thread calls the layout entry points.  A record:
 *   word 0      NP_LAYOUT_FAMILY: NP_LAYOUT_PATH_*
 *   word 1      NP_LAYOUT_FORM: the template arguments — INTERLEAVE: R | TO_INTERLEAVED << 8; SKINNY: TALL; TILE: tile | VEC << 8;
 *               WALIGN: tile; PLANE: W; GATHER: index bits (32 / 64) | W << 8; COPY2D: V; MEMCPY: 0
 *   word 2      NP_LAYOUT_ORDER: the tile order as passed to the kernel (TILE 0 / 1, WALIGN 0 / 1 / 2, PLANE its xcd_runs; else 0)
 *   words 3-5   NP_LAYOUT_GRID_X / _Y / _Z: the grid (0, 0, 0 for MEMCPY)
 *   words 6-14  by family, 0 where unused — TILE and WALIGN: tiles_x, tiles_y, in_pitch, out_pitch (floats, low 32 bits), nbatch
 *               (batch axes in the PlaneBatch); PLANE: A, B, E, ta, tb, tiles_a, tiles_b, pitch, xcd_runs as the kernel sees them
 *               (float4 units where W = 4) */
#define NP_LAYOUT_RECORD_WORDS 16u
#define NP_LAYOUT_FAMILY 0
#define NP_LAYOUT_FORM 1
#define NP_LAYOUT_ORDER 2
#define NP_LAYOUT_GRID_X 3
#define NP_LAYOUT_GRID_Y 4
#define NP_LAYOUT_GRID_Z 5
#define NP_LAYOUT_EXTRA 6
#define NP_LAYOUT_PATH_NONE 0u
#define NP_LAYOUT_PATH_MEMCPY 1u       /* np_memcpy_d2d: identity after fusion, contiguous strides, unpitched np_copy2d */
#define NP_LAYOUT_PATH_INTERLEAVE 2u   /* interleave_kernel<R, TO_INTERLEAVED> */
#define NP_LAYOUT_PATH_SKINNY 3u       /* transpose_skinny_kernel<TALL> */
#define NP_LAYOUT_PATH_TILE 4u         /* transpose_tile_kernel<T, T, VEC> */
#define NP_LAYOUT_PATH_WALIGN 5u       /* transpose_walign_kernel<T, T> */
#define NP_LAYOUT_PATH_PLANE 6u        /* permute_plane_kernel<W> */
#define NP_LAYOUT_PATH_GATHER 7u       /* permute_gather_kernel<I, W> */
#define NP_LAYOUT_PATH_COPY2D 8u       /* copy2d_kernel<V> */
int np_debug_layout_last_record(unsigned *host_record, unsigned capacity, unsigned *host_count);
/* tests / tools: what the last np_argreduce call of the process launched: ONE record of NP_ARG_RECORD_WORDS unsigned words naming the
 * streaming kernel and the fold of its partials.  Cleared at the top of np_argreduce; the early returns (outer == 0, inner == 0) and
 * the refusals leave it cleared: *host_count = 0 then, else 1.  `capacity` counts records: min(count, capacity) records are written.
 * Host stores at the launch sites: no device work, no synchronisation, no kernel argument; plain process globals, meaningful only
 * while one thread calls np_argreduce.  A record:
 *   word 0      NP_ARG_KERNEL: NP_ARG_KERNEL_*, the streaming kernel
 *   word 1      NP_ARG_TEMPLATE: its template argument besides IS_MAX — ROWS_GROUP: L; COLS_TILE: FINAL; else 0
 *   words 2-4   NP_ARG_GRID_X / _Y / _Z: its grid
 *   word 5      NP_ARG_CHUNKS: the pieces the axis is cut into (slabs of the flat walks, chunks of ROWS, COLS_TILE and CHUNKS; 1 for
 *               the kernels that write the result themselves)
 *   word 6      NP_ARG_CHUNK_LEN: elements of the axis per piece (rows_per_block of the flat walks; the axis itself where chunks = 1
 *               except COLS_TILE, which reports the chunk_len it passes)
 *   word 7      NP_ARG_XCD_RUNS: COLS_TILE's xcd_runs argument, else 0
 *   word 8      NP_ARG_FOLD: NP_ARG_FOLD_*, the kernel that folds the partials (NONE: the streaming kernel wrote the indices)
 *   word 9      NP_ARG_FOLD_COLS: COLS of argreduce_fold_cols_kernel, else 0
 *   words 10-12 NP_ARG_FOLD_GRID_X / _Y / _Z: the fold's grid (0, 0, 0 without one) */
#define NP_ARG_RECORD_WORDS 16u
#define NP_ARG_KERNEL 0
#define NP_ARG_TEMPLATE 1
#define NP_ARG_GRID_X 2
#define NP_ARG_GRID_Y 3
#define NP_ARG_GRID_Z 4
#define NP_ARG_CHUNKS 5
#define NP_ARG_CHUNK_LEN 6
#define NP_ARG_XCD_RUNS 7
#define NP_ARG_FOLD 8
#define NP_ARG_FOLD_COLS 9
#define NP_ARG_FOLD_GRID_X 10
#define NP_ARG_FOLD_GRID_Y 11
#define NP_ARG_FOLD_GRID_Z 12
#define NP_ARG_KERNEL_NONE 0u
#define NP_ARG_KERNEL_ROWS_GROUP 1u     /* argreduce_rows_group<L> */
#define NP_ARG_KERNEL_ROWS_WAVE 2u      /* argreduce_rows_wave */
#define NP_ARG_KERNEL_ROWS 3u           /* argreduce_rows_kernel */
#define NP_ARG_KERNEL_SMALL_INNER 4u    /* argreduce_small_inner */
#define NP_ARG_KERNEL_SMALL_INNER4 5u   /* argreduce_small_inner4 */
#define NP_ARG_KERNEL_COLS_TILE 6u      /* argreduce_cols_tile<FINAL> */
#define NP_ARG_KERNEL_CHUNKS 7u         /* argreduce_chunks_kernel */
#define NP_ARG_KERNEL_GENERIC 8u        /* argreduce_generic_kernel */
#define NP_ARG_FOLD_NONE 0u
#define NP_ARG_FOLD_THREAD 1u           /* argreduce_fold_kernel, a thread per output */
#define NP_ARG_FOLD_BLOCK 2u            /* argreduce_fold_block_kernel, a workgroup per output */
#define NP_ARG_FOLD_COLS_KERNEL 3u      /* argreduce_fold_cols_kernel<COLS> */
int np_debug_argreduce_last_record(unsigned *host_record, unsigned capacity, unsigned *host_count);

#ifdef __cplusplus
}
#endif

#endif /* NUMPOWER_AMD_NP_HIP_DEBUG_H */
