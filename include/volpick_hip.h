/*
 * volpick_hip.h — C ABI of libvolpick_hip.so, the MI355X (gfx950) implementation of
 * volpick's sliding-window phase-picking inference path.
 *
 * The reference reaches this path through a Python object API, not an FFI
 * (SURVEY.md §8b): seisbench.models.{PhaseNet,EQTransformer} instances created with
 * from_pretrained("volpick") and driven by classify()/annotate()/__call__
 * (the reference's README.md:46-66, Final_models/demo.ipynb:300-301,359-360,397-398,
 * volpick/model/eval_taks0.py:58-89).  Each entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only; no torch types.
 *
 * Conventions: every function returns 0 on success or a negative vp_status;
 * vp_last_error() returns a thread-local message.  Handles are opaque; one handle is
 * bound to one HIP device and one HIP stream and is used from one thread at a time.
 * "dev" pointers are HIP device pointers on the handle's device, "host" pointers are
 * ordinary host memory.  All floats are IEEE fp32.
 */
#ifndef VOLPICK_HIP_H
#define VOLPICK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vp_handle vp_handle;

typedef enum {
  VP_OK = 0,
  VP_ERR_INVALID = -1,   /* bad argument */
  VP_ERR_HIP = -2,       /* a HIP runtime call failed */
  VP_ERR_NOMEM = -3,     /* workspace too small / allocation failed */
  VP_ERR_UNSUPPORTED = -4
} vp_status;

enum { VP_MODEL_PHASENET = 0, VP_MODEL_EQTRANSFORMER = 1 };
enum { VP_NORM_PEAK = 0, VP_NORM_STD = 1 };
enum { VP_STACK_AVG = 0, VP_STACK_MAX = 1 };
enum { VP_MEM_HOST = 0, VP_MEM_DEVICE = 1 };

/* Constants the reference does not pin; defaults are the
 * published SeisBench values, filled in by vp_default_config(). */
typedef struct {
  int32_t norm;               /* VP_NORM_*  — model_args.norm, Final_models/ ** /volpick.json.v1:6 */
  int32_t norm_amp_per_comp;  /* EQT only: 1 = per-channel PEAK amplitude (whatever `norm` says, as SeisBench's
                                 annotate_batch_pre), 0 = one peak / std amplitude over all channels */
  int32_t max_batch;          /* windows the workspace is sized for per forward pass */
  float bn_eps;               /* BatchNorm eps, folded into the conv weights at load time */
  float attention_eps;        /* EQT additive attention denominator eps */
  float layernorm_eps;        /* EQT LayerNormalization eps */
  float norm_eps;             /* x / (amp + norm_eps) */
  int32_t taper_samples;      /* EQT half-cosine taper length (0 for PhaseNet) */
  int32_t plan_flags[8];      /* plan selectors (debug plans, A/B timing; all 0 = the default plan; the library's names for
                                 every index, value and bit: volpick_amd/csrc/plan_flags.h):
                                 [0]: 1 = PhaseNet layer-by-layer plan instead of the fused kernels (debug / A-B);
                                 [1]: bit0 = fused kernels also dump their LDS intermediates to the debug tensors
                                      (selects the three-launch plan), bit1 = per-layer clock stamps,
                                      bit2 = PhaseNet: the one-launch kernel's DUMP instance writes every layer's output and
                                      the head's logits to the debug tensors (tests; rejected with bit0, [5] or [6] set);
                                      EQTransformer: the DUMP instances of the five default conv kernels write every conv
                                      layer's output (encoder.0-5, res.{i}.mid / .conv2 / .out, decoder.0-6 and the heads'
                                      logits, the decoders' set-major) to the debug tensors; the decoder tail computes whole
                                      rows in 1200-sample tiles; the DUMP instance of eqt_mid4 writes every stage of the
                                      BiLSTM blocks, the transformers and the pick branches (bilstm.{i}.h / .c, transformer
                                      .p / .att / .y1 / .ff1 / .ff2, pick_lstms.{k}.h / .c, pick_attentions.{k}.p) (tests;
                                      rejected with [0], [2], [3] or any [7] bit but bit10 set, or [6] = 2);
                                 [2]: PhaseNet: (1 = hand-pipelined K loop in the MFMA layers: removed in round 6, rejected);
                                      EQTransformer: 1 = the three
                                      BiLSTM blocks, two transformer blocks and the pick branches as six launches instead
                                      of the one-launch middle kernel (the independent reference: scalar FMA chains),
                                      2 = the one-launch kernel with ONE window per 256-thread workgroup (the bit reference
                                      of the tests); default: eqt_mid4_kernel, FOUR windows per 1024-thread workgroup in
                                      teams of four waves, so that a batch of 256 holds 64 CUs and leaves the rest to the
                                      kernels of the other device contexts (bit-identical to 2); (3, two windows per
                                      workgroup in teams of eight waves, was removed and is rejected);
                                 [3]: PhaseNet: 1 = the tiled level-0 up kernel of the three-launch plans with one workgroup
                                      per tile (A/B; 2, the persistent down kernel, was removed in round 6); EQTransformer:
                                      (1, half-width tiles for decoder stages 3-6, was removed and is rejected); 64 = PhaseNet's one-launch plan
                                      WITHOUT the first-come-first-served gate between the device contexts' forward
                                      launches (A/B: csrc/api.hip ForwardGate);
                                 [4]: 1 = no L2 warm-up of the weight streams;
                                 [5]: PhaseNet plan: 0 = the whole network in one launch, its five deepest layers on the
                                      bf16 matrix cores with exact three-piece operands (default), 1 = three launches,
                                      all MFMA (bit-identical to the layer plan), 2 = three launches, level-0
                                      stride-1 convs on the VALU, 3 = one launch, every core layer on the fp32 MFMA
                                      (the reference of the bf16-piece layers), 8 = one launch with inc and down0.same
                                      as packed-FMA direct convolutions on the vector ALUs and up3.convT / up3.same /
                                      head in round 4's forms (the rounding reference of the tiled level-0 layers);
                                      4, 5, 6, 7, 9 -- intermediate forms of rounds 2-5 -- were removed in round 6 and
                                      are rejected (default: all of these on the bf16 matrix cores too -- up1.same /
                                      up2.same in two K halves over one piece image that is refilled in between, inc /
                                      down0.same time-tiled in six tiles of 512 samples, up3.convT / up3.same / head in
                                      twelve tiles of 256 with producer and consumer waves);
                                 [6]: PhaseNet: 1 = the one-launch plan reads the input tensor filled by gather_normalize
                                      instead of cutting and normalising its windows itself; EQTransformer: 2 = the fused
                                      encoder front cuts and normalises its windows itself (A/B: slower end to end);
                                 [7]: EQTransformer: bit0 = decoder stages 4-6 + heads as three launches instead of the
                                      time-tiled fused kernel, bit1 = decoder stages 0-3 as five launches instead of one
                                      per-row fused kernel, bit2 = encoder stages 0-2 as three launches instead of the
                                      time-tiled fused kernel, bit3 = encoder stages 3-6 as four launches instead of one
                                      per-window fused kernel (all bit-identical; layer tests, A/B timing),
                                      bit4 = the fused ResCNN kernel, bit5 = stages 1 and 2 of the fused decoder 0-3
                                      kernel, bit6 = the fused decoder tail (stages 4-6 + heads), bit7 = the fused encoder 3-6 kernel, bit8 = stages 1 and 2 of the fused encoder 0-2 kernel on the fp32 MFMA
                                      instead of the bf16 matrix cores with exact three-piece operands (the two
                                      forms agree to fp32 rounding, not bitwise), bit9 = the bf16-piece ResCNN kernel with
                                      four waves per window and ONE window per 256-thread workgroup,
                                      bit10 = the decoder tail computes every tile of a row even where annotate / classify
                                      blind the output (default: only the tiles that hold kept samples),
                                      bit11 = stage 3 of the fused decoder 0-3 kernel shares its n-tiles evenly between
                                      the two waves of a SIMD (default: 14 + 10),
                                      (default ResCNN kernel: eqt_res3t_kernel, eight waves per THREE windows, a wave taking 16
                                      output channels of five or four of the nine n-tiles; bit-identical to bit9),
                                      (bit12, the bf16-piece ResCNN kernel with eight waves per window and K split over
                                      wave pairs, was removed in round 6 and is rejected; so is bit13, the same kernel as
                                      bit9 with TWO windows per 512-thread workgroup) */
  int32_t reserved[4];        /* must be 0 */
} vp_config;

/* Fills cfg with the defaults for model_kind. */
int vp_default_config(int model_kind, vp_config* cfg);

/* Number of fp32 values vp_create expects in `weights` for model_kind, and the canonical
 * tensor order: the state-dict order of Final_models/ ** / *.pt.v1 without the
 * num_batches_tracked entries.  vp_param_name/vp_param_size
 * enumerate it (index 0..vp_param_count-1). */
size_t vp_weight_count(int model_kind);
int vp_param_count(int model_kind);
const char* vp_param_name(int model_kind, int index);
size_t vp_param_size(int model_kind, int index);

/* Replaces sbm.<Model>.from_pretrained(name) + model.cuda()  (README.md:46-47,
 * demo.ipynb:224-227): builds the device plan (BN folding, MFMA fragment packing),
 * uploads it and allocates the workspace.  weights_mem says where `weights` lives
 * (VP_MEM_DEVICE after vp_bcast-style distribution). */
int vp_create(int device_id, int model_kind, const float* weights, size_t n_floats, int weights_mem,
              const vp_config* cfg, vp_handle** out);
int vp_destroy(vp_handle* h);

/* Geometry of the model behind the handle. */
int vp_in_samples(const vp_handle* h);   /* 3001 (PhaseNet) / 6000 (EQTransformer) */
int vp_n_outputs(const vp_handle* h);    /* 3: PhaseNet (P,S,N in `phases` order) / EQT (Detection,P,S) */

/* Replaces model(x) under torch.no_grad()/model.eval() on a (B,3,T) float32 tensor
 * (volpick/model/eval_taks0.py:58-61,69,86).  x: B*3*T, y: B*n_out*T, both in the memory
 * space x_mem/y_mem.  preprocess != 0 additionally applies annotate_batch_pre
 * (demean + amplitude normalisation [+ taper]) to each window first.
 * B may exceed max_batch; it is processed in chunks. */
int vp_forward(vp_handle* h, const float* x, int x_mem, int B, int preprocess, float* y, int y_mem);

/* Replaces WaveformModel.annotate on one station block (call
 * stack §3.1): windows of in_samples at stride in_samples-overlap plus one tail window,
 * annotate_batch_pre, forward, NaN blinding, overlap stacking (avg / max).
 * stream: 3*N samples, rows in component_order.  out: n_out*N, NaN where no un-blinded
 * window covers a sample.  first_valid/last_valid (may be NULL): the NaN-trimmed range
 * [first_valid, last_valid] of output row 0; first_valid = -1 if nothing is valid.
 * Returns the number of windows in *n_windows (may be NULL).  N < in_samples yields an
 * all-NaN output and 0 windows (the reference only warns). */
int vp_annotate(vp_handle* h, const float* stream, int stream_mem, int64_t N, int overlap, int blind_l,
                int blind_r, int stacking, int batch, float* out, int out_mem, int64_t* first_valid,
                int64_t* last_valid, int64_t* n_windows);

/* Replaces obspy trigger_onset + per-trigger max/argmax as used by
 * picks_from_annotations / detections_from_annotations and by the reference's own
 * get_picks_from_prob (volpick/model/eval_taks0.py:46-56).  trace: n samples (may hold
 * NaN).  A trigger opens at the first sample > thr_on and closes at the last sample of
 * the run of samples > thr_off.  Writes the earliest (by onset) min(cap, total) triggers in onset order;
 * *n_found is the total. */
int vp_pick(vp_handle* h, const float* trace, int trace_mem, int64_t n, float thr_on, float thr_off,
            int64_t* on, int64_t* off, int64_t* peak, float* value, int cap, int* n_found);

/* Replaces model.classify(stream, ...) on one station block (README.md:54-66): vp_annotate
 * followed by the trigger/peak scan of the output rows named in `specs`, with a single
 * host synchronisation and a single device->host copy of the triggers.  `out` may be NULL
 * (annotations not wanted), a device buffer or a host buffer of n_out*N floats.  Triggers
 * are indices into the N-sample output rows (not the NaN-trimmed traces), grouped by spec in
 * spec order and sorted by onset inside each group; spec_of[i] (may be NULL) is the spec
 * index of trigger i.  Requires thr_off <= thr_on. */
typedef struct {
  int32_t row;     /* output row: PhaseNet 0..2 in `phases` order; EQT 0 Detection, 1 P, 2 S */
  float thr_on;    /* trigger opens at the first sample > thr_on */
  float thr_off;   /* ... and closes at the last sample of the run of samples > thr_off */
} vp_trigger_spec;
int vp_classify(vp_handle* h, const float* stream, int stream_mem, int64_t N, int overlap, int blind_l,
                int blind_r, int stacking, int batch, const vp_trigger_spec* specs, int n_specs, float* out,
                int out_mem, int64_t* first_valid, int64_t* last_valid, int64_t* n_windows, int64_t* on,
                int64_t* off, int64_t* peak, float* value, int32_t* spec_of, int cap, int* n_found);

/* The trigger scan of vp_classify alone: `rows_dev` is a device (n_out, N) array of stacked rows (what vp_annotate left
 * there); every spec's row is scanned in one launch, one synchronisation, one result copy.  Same result layout and cap
 * rule as vp_classify. */
int vp_pick_rows(vp_handle* h, const float* rows_dev, int64_t N, const vp_trigger_spec* specs, int n_specs, int64_t* on,
                 int64_t* off, int64_t* peak, float* value, int32_t* spec_of, int cap, int* n_found);

/* Asynchronous form of vp_classify for callers that keep the GPU fed (several station blocks
 * or bench steps in flight): vp_classify_submit enqueues the whole path on the handle's stream
 * and returns without synchronising; vp_classify_collect(slot) waits for that submit and returns
 * its triggers.  Up to VP_MAX_INFLIGHT submits may be outstanding, each in its own slot; work is
 * executed in submit order.  Buffers passed to submit (stream, out) must stay valid until the
 * matching collect; a device `out` shared by several in-flight submits is overwritten in order. */
#define VP_MAX_INFLIGHT 4
int vp_classify_submit(vp_handle* h, int slot, const float* stream, int stream_mem, int64_t N, int overlap,
                       int blind_l, int blind_r, int stacking, int batch, const vp_trigger_spec* specs, int n_specs,
                       float* out, int out_mem, int cap);
int vp_classify_collect(vp_handle* h, int slot, int64_t* first_valid, int64_t* last_valid, int64_t* n_windows,
                        int64_t* on, int64_t* off, int64_t* peak, float* value, int32_t* spec_of, int cap,
                        int* n_found);

/* Replaces the per-sample loop of the reference's own evaluation protocol
 * (volpick/model/eval_taks0.py:46-56,96-142: get_picks_from_prob on window_borders slices).
 * prob: (B, n_rows, T) model outputs; for window b the samples [lo[b], hi[b]) of channel `row`
 * are scanned (lo/hi NULL = whole window).  Per window up to K triggers are returned, unordered:
 * peak[b*K + i] = argmax index relative to lo[b], value[b*K + i] = the maximum; count[b] is the
 * number found (may exceed K).  The reference calls this with thr_off = thr_on / 2. */
int vp_pick_windows(vp_handle* h, const float* prob, int prob_mem, int B, int n_rows, int row, const int32_t* lo,
                    const int32_t* hi, float thr_on, float thr_off, int K, int32_t* count, int32_t* peak,
                    float* value);

/* vp_classify over K stream blocks (stations / contiguous segments) in ONE call: the windows of all blocks
 * share the forward batches -- SeisBench's batch_size spans every fragment of the stream it is given
 * (the reference's README.md:54-66) -- and stacking and the trigger scan are one launch each.
 * `streams` (host or device) holds block k as 3 rows of lengths[k] samples at float offset offsets[k];
 * `out` (may be NULL) receives the stacked rows in the same layout.  first_valid / last_valid / n_windows
 * are arrays of K.  Triggers come back grouped by block, then spec, sorted by onset, with block_of /
 * spec_of; every (block, spec) row has room for cap_per_row triggers on the device.  *n_found > cap (or a row
 * with more than cap_per_row triggers) means: call again with more room. */
int vp_classify_multi(vp_handle* h, const float* streams, int stream_mem, const int64_t* offsets,
                      const int64_t* lengths, int K, int overlap, int blind_l, int blind_r, int stacking, int batch,
                      const vp_trigger_spec* specs, int n_specs, float* out, int out_mem, int64_t* first_valid,
                      int64_t* last_valid, int64_t* n_windows, int64_t* on, int64_t* off, int64_t* peak, float* value,
                      int32_t* spec_of, int32_t* block_of, int cap_per_row, int cap, int* n_found);

/* Host-only variant of vp_pick for traces already in host memory (no handle, no GPU). */
int vp_pick_host(const float* trace, int64_t n, float thr_on, float thr_off, int64_t* on, int64_t* off,
                 int64_t* peak, float* value, int cap, int* n_found);

/* Window start rule of the reference.  Writes up to cap starts,
 * returns the count (0 if N < in_samples), negative on bad arguments. */
int64_t vp_window_starts(int64_t N, int in_samples, int overlap, int64_t* starts, int64_t cap);

/* Timing of the last vp_forward / vp_annotate on this handle, measured with HIP events on
 * the handle's stream (only while vp_set_timing(h, 1) is in effect): total milliseconds and the per-stage split
 * (0 preprocess, 1 model forward, 2 blinding+stacking, 3 pick scan). */
int vp_last_timing(const vp_handle* h, float* total_ms, float stage_ms[4]);
/* Stage events are OFF by default (each hipEventRecord opens a ~5 us bubble on the stream);
 * enable them for the calls whose vp_last_timing split is wanted. */
int vp_set_timing(vp_handle* h, int enable);

/* The handle's HIP stream (hipStream_t) for callers that want to order their own work. */
void* vp_stream(const vp_handle* h);
int vp_synchronize(vp_handle* h);

/* Introspection for bench.py: the forward pass is a fixed list of kernel launches
 * ("steps").  vp_step_info gives a step's name and its ALGORITHMIC flop count per window
 * (2*MAC of the layer it implements, not the padded MFMA work); vp_flops_per_window is
 * their sum.  vp_profile_steps runs each launch `iters` times on B windows and reports its
 * mean duration in ms, measured with HIP events on the handle's stream. */
int vp_step_count(const vp_handle* h);
int vp_step_info(const vp_handle* h, int index, const char** name, double* flops_per_window);
double vp_flops_per_window(const vp_handle* h);
/* The work a launch actually issues per window (whole 16-column tiles, channels padded to 4, recomputed halos, the
 * folded taps of the polyphase forms), as fp32-equivalent FLOP. */
int vp_step_issued_flops(const vp_handle* h, int index, double* issued_flops_per_window);
/* The same work by the pipe it is issued to -- what a roofline of the launch has to be priced with: FLOP per window as
 * fp32 MFMAs (v_mfma_f32_16x16x4_f32), as bf16 MFMAs (v_mfma_f32_16x16x32_bf16; an exact three-piece product is SIX of
 * them, all counted) and on the vector ALUs (direct convolutions, recurrences, attention scores).  Filled for every
 * launch of every plan; vp_step_issued_flops = mfma_f32 + mfma_bf16 / 6 + valu (its fp32 equivalent). */
typedef struct {
  double mfma_f32_flop, mfma_bf16_flop, valu_flop;
} vp_issued_work;
int vp_step_issued_work(const vp_handle* h, int index, vp_issued_work* out);
/* A launch whose tiling follows the output range the caller keeps (eqt_tail3_kernel: only the tiles that hold un-blinded
 * samples) issues different work for different ranges.  vp_step_issued_work answers for the range the vp_profile_* calls
 * time (the one the handle's latest preprocessing batch kept); this one for any [out_lo, out_hi) (out_hi <= 0: the whole
 * row, what model(x) computes).  Pure: no launch changes what either reports. */
int vp_step_issued_work_for_range(const vp_handle* h, int index, int out_lo, int out_hi, vp_issued_work* out);
int vp_profile_steps(vp_handle* h, int B, int iters, float* step_ms, int cap);
/* One step timed IN the pipeline: the whole list runs in order `iters` times, only step `index` is bracketed by
 * events (its inputs come from the preceding kernel, as under rocprofv3). */
int vp_profile_step_in_pipeline(vp_handle* h, int B, int iters, int index, float* ms);
/* launch `index` alone, iters times back to back (two handles on two host threads: do two kernels share the chip?) */
int vp_profile_one_step(vp_handle* h, int B, int iters, int index, float* ms);

/* Host-only (no GPU): plans the model and returns conv layer `conv_index`'s geometry
 * (13 ints: cin1,cin2,cout,P,taps,sn,in_off,out_off,waves_m,waves_n,nw,relu,epi), packed
 * MFMA A-fragments and folded bias.  Returns the fragment float count, or -(1000 + number
 * of conv layers) when conv_index is out of range.  Used by the CPU tests of BN folding and
 * fragment packing. */
int vp_debug_plan_conv(int model_kind, const float* weights, size_t n_floats, const vp_config* cfg,
                       int conv_index, int* geom13, float* afrag, size_t afrag_cap, float* bias, size_t bias_cap,
                       const char** name, int* cols, int* l_out);

/* Debug: number of intermediate activation tensors of the last forward pass and a copy of
 * one of them as a dense (B, C, L) host array (used by the layer-by-layer parity tests). */
int vp_debug_tensor_count(const vp_handle* h);
int vp_debug_tensor_info(const vp_handle* h, int index, const char** name, int* channels, int* length);
int vp_debug_tensor_read(vp_handle* h, int index, int B, float* host_out);  /* VP_ERR_UNSUPPORTED: the plan keeps it in LDS */

/* Debug guard of the data-layout invariant the conv loaders rely on: the margins of every
 * activation row -- [0, 8) and [8 + L, row stride) -- are the convolution padding, zeroed once at vp_create and never
 * written again.  Scans every row of every tensor; *n_bad = margin words that are not +-0.0, *first_bad_tensor (may be
 * NULL) the name of the first offending tensor.  Meant to be run after calls on ragged sizes.  self_test = k > 0 plants
 * one stray word in a margin of tensor k - 1 for the duration of the scan (the checker checking itself: expect 1). */
int vp_debug_check_halos(vp_handle* h, int self_test, int64_t* n_bad, const char** first_bad_tensor);

/* Debug (handles created with plan_flags[1] & 2): B x 32 words per window of the fused PhaseNet core
 * kernel: [0..14] shader-clock stamps (kernel start, input loaded, after each of the 13 layers),
 * [16],[17] the 100 MHz wall clock at kernel start / end, [18..22] phase stamps of pn_up3p_kernel. */
int vp_debug_core_clock(vp_handle* h, int B, unsigned long long* out32);
/* Same flag: 8 stamps per conv_mfma_kernel launch (in plan order of the conv layers) of one probe
 * workgroup: start, input staged, MFMA loop done, output staged, stored.  Returns the layer count. */
int vp_debug_conv_clock(vp_handle* h, unsigned long long* out, int max_layers);
/* Same flag, EQTransformer: B x 32 words of eqt_tail_kernel, one row per workgroup: six stamps for each of its first
 * four tiles (tile start, image parked, after stage 4 / 5 / 6, heads done); [24], [25] the shader clock and [30], [31] the
 * 100 MHz wall clock at kernel start / end. */
int vp_debug_tail_clock(vp_handle* h, int B, unsigned long long* out32);

/* ---------------------------------------------------------------------------------------------
 * Waveform-file ingestion: miniSEED 2 and miniSEED 3 records -> sample arrays,
 * the step the reference performs with obspy.read() (libmseed) before stream_to_array
 * (the reference's volpick/data/convert.py:7,26-70).
 *
 * vp_mseed_scan (host only, no GPU) walks a miniSEED byte string and fills one vp_mseed_record per
 * data record; the two formats may be mixed in one buffer.  miniSEED 2: fixed header, blockette 1000
 * (encoding, word order, record length) and blockette 1001 (microseconds); the header time
 * correction is applied unless activity flag bit 1 says it already was.  miniSEED 3 (FDSN 2020:
 * "MS" 3, 40-byte little-endian fixed header, source identifier "FDSN:NET_STA_LOC_B_S_SS", extra
 * headers, payload): the CRC-32C of every record is verified (VP_ERR_INVALID on a mismatch), start
 * times are truncated from nanoseconds to microseconds, a negative rate field is a period in
 * seconds, the channel is BAND SOURCE SUBSOURCE joined when each is one character; identifiers whose
 * codes do not fit the fields below are VP_ERR_UNSUPPORTED.  Writes at most `cap` records and always
 * reports the total in *n_found.
 *
 * vp_mseed_decode (HIP, one wavefront per record) decodes records into `out`: record r's samples go
 * to out[out_index[r] .. out_index[r] + min(nsamples, out_count[r])), clipped to [0, out_len);
 * out_index[r] < 0 skips the record, out_count may be NULL.  Encodings: 0 text (one sample per byte,
 * its unsigned value), 1 int16, 2 int24, 3 int32, 4 float32, 5 float64, 10 Steim-1, 11 Steim-2,
 * either byte order.  out_kind VP_SAMPLES_INT32 (integer
 * encodings only, exact) or VP_SAMPLES_FLOAT32.  zero_fill != 0 clears `out` first (the zero fill of
 * gaps in stream_to_array).  `status` (host, may be NULL) receives per record 0 = ok,
 * 1 = Steim reverse-integration constant mismatch, 2 = payload shorter than the header's count.
 * buf / out may be host or device memory (buf_mem / out_mem); recs, out_index, out_count, status
 * are host arrays.  buf itself must be 4-byte aligned; payloads may start at any byte (miniSEED 3
 * headers have no fixed length). */
enum { VP_SAMPLES_INT32 = 0, VP_SAMPLES_FLOAT32 = 1 };
typedef struct {
  int64_t offset;      /* byte offset of the record */
  int64_t start_us;    /* first sample, microseconds since 1970-01-01T00:00:00 UTC */
  double sample_rate;  /* Hz */
  int32_t reclen, data_offset, nsamples, encoding;
  int32_t big_endian;  /* word order of the payload (and of a miniSEED 2 header) */
  int32_t quality;     /* miniSEED 2: data quality indicator character; miniSEED 3: 0x300 | publication version */
  char network[4], station[8], location[4], channel[4]; /* NUL terminated, blanks stripped */
} vp_mseed_record;
int vp_mseed_scan(const uint8_t* buf, size_t nbytes, vp_mseed_record* recs, int64_t cap, int64_t* n_found);
int vp_mseed_decode(int device_id, const uint8_t* buf, int buf_mem, size_t nbytes, const vp_mseed_record* recs,
                    const int64_t* out_index, const int64_t* out_count, int64_t n_recs, int out_kind, void* out,
                    int out_mem, int64_t out_len, int zero_fill, int32_t* status);
/* vp_mseed_scan_segments (host only, no GPU, callable from any thread: vp_mseed_scan's class) is vp_mseed_scan plus the
 * bookkeeping a reader does next: the records with samples (nsamples > 0) are put in the order (network, station, location,
 * channel, start_us, offset) and chained into continuous segments by libmseed's trace-list rule -- a record extends the
 * previous one's segment when id, rate and sample kind (float encodings 4 / 5 against the rest) are the same and it starts one
 * period after that record's last sample, within half a period.  recs[0 .. *n_kept) is the ordered table and seg[i] the
 * segment number of recs[i] (from 0, non-decreasing); `seg` holds `cap` words.  *n_found is vp_mseed_scan's total: when it
 * exceeds `cap` nothing was ordered (*n_kept = 0) and the call is to be repeated with room.  Errors are vp_mseed_scan's. */
int vp_mseed_scan_segments(const uint8_t* buf, size_t nbytes, vp_mseed_record* recs, int64_t* seg, int64_t cap,
                           int64_t* n_found, int64_t* n_kept);
/* vp_mseed_decode for a pipeline: the same kernel and the same record checks, enqueued on the caller's `stream` (a
 * hipStream_t, not the null stream) and never waited for.  buf_dev (4-byte aligned, nbytes rounded up to a whole word
 * readable), out_dev (out_len samples of out_kind) and status_dev are device memory; recs, out_index, out_count are host
 * arrays read before the call returns.  Records are skipped as in vp_mseed_decode (out_index[r] < 0, nsamples <= 0); the
 * others -- *n_decoded of them, in table order -- get one status word each, status_dev[0 .. *n_decoded), with
 * vp_mseed_decode's values.  out_count[r] = 0 decodes a record for its status alone.  The launch table travels through
 * memory of the caller's: table_host (page-locked, to stay untouched until the copy has run on `stream`) and table_dev
 * (until the kernel has), each table_bytes >= VP_MSEED_TABLE_BYTES_PER_RECORD * n_recs.  Holds no lock and no scratch: any
 * number of calls may be in flight, on any streams.  With out_index[r] = row * N + offset, VP_SAMPLES_FLOAT32 and
 * zero_fill it writes a station's (C, N) float32 block -- gap fill, missing components and component order -- in one launch. */
enum { VP_MSEED_TABLE_BYTES_PER_RECORD = 32 };
int vp_mseed_decode_on(int device_id, const uint8_t* buf_dev, size_t nbytes, const vp_mseed_record* recs,
                       const int64_t* out_index, const int64_t* out_count, int64_t n_recs, int out_kind, void* out_dev,
                       int64_t out_len, int zero_fill, int32_t* status_dev, void* table_host, void* table_dev,
                       size_t table_bytes, int64_t* n_decoded, void* stream);
/* Mean kernel time (ms, HIP events) of `iters` decodes of the same device-resident inputs: bench only. */
int vp_mseed_decode_bench(int device_id, const uint8_t* buf_dev, size_t nbytes, const vp_mseed_record* recs,
                          const int64_t* out_index, int64_t n_recs, int out_kind, void* out_dev, int64_t out_len,
                          int iters, float* ms);
/* vp_mseed_decode keeps its device scratch (file image, sample array of host destinations, record table: ~175 MB after one
 * host-to-host station-day) per device, grow-only, for the life of the process, and serialises the calls on one device from
 * their first use of it to their final stream synchronisation.  This frees it (waits for a call in flight; the next decode
 * allocates again).  bytes_freed may be NULL.  No counterpart in the reference (obspy.read holds no device memory). */
int vp_mseed_release_scratch(int device_id, size_t* bytes_freed);

/* ---------------------------------------------------------------------------------------------
 * Traces to miniSEED: the other direction, the reference's waveforms.write(path, format="MSEED")
 * (volpick/data/data.py:1353).  miniSEED 2 only: records of `reclen` bytes (a power of two in 128..65536) with the fixed
 * header, blockette 1000 at byte 48, an optional blockette 1001 at byte 56 and the data at byte 64; traces in the order
 * given, record after record, sequence numbers from 1 through the whole output.
 *
 * vp_mseed_encode packs the samples of `n_traces` traces: trace t is samples[first_sample .. first_sample + nsamples) of
 * `samples` (host or device memory, samples_mem; elements of sample_kind, a VP_SAMPLES_* value; `first_sample` may be any
 * element offset from the base, so traces in separate device arrays are read where they lie).  Encodings by sample kind:
 * int32 -> 11 (Steim-2), 10 (Steim-1), 3 (int32), 1 (int16); float32 -> 4; float64 -> 5.  Steim words are packed greedily
 * over the differences d[i] = x[i] - x[i-1] (wrapped to int32, x[-1] = 0 at the start of a trace): the first option that
 * still has enough differences left in the trace and fits all of them wins -- Steim-2: 7x4, 6x5, 5x6, 4x8, 3x10, 2x15, 1x30
 * bits; Steim-1: 4x8, 2x16, 1x32 -- and a record holds 15 * (reclen / 64 - 1) - 2 data words behind X0 and Xn; unused words of
 * a trace's last record are zero.  The first difference of a trace is stored as 0 under Steim-2 when x[0] does not fit 30
 * bits (decoders start from X0).  Any other Steim-2 difference outside 30 bits, and an int32 sample outside int16 under
 * encoding 1, refuses the whole call: VP_ERR_INVALID, *bad_trace and *bad_sample name the first trace with such a sample and
 * its lowest offending index (otherwise both are -1), nothing is written.  Float bits pass unchanged.
 * b1001_mode: 0 never, 1 always, -1 for every record of a trace as soon as one record of that trace starts at a time that
 * is no multiple of 100 microseconds.  A record that starts at sample `pos` starts at start_us + nearbyint(pos * 1e6 /
 * sample_rate) (halves to even).  Traces with nsamples <= 0 are skipped.
 * The output goes to out_host (host memory, out_cap bytes); *out_bytes and *n_records are always reported, and when
 * *out_bytes > out_cap nothing is written and the call is to be repeated with room (vp_mseed_scan's idiom; (number of
 * traces + total samples / samples per record at one difference per word) records are always enough).
 * VP_ERR_INVALID: a null pointer, a bad kind / encoding / reclen / rate (vp_mseed_rate_fields refuses it), a code longer
 * than its header field.  VP_ERR_UNSUPPORTED: a record could hold more than 65535 samples (Steim-2 at 65536 bytes).  Runs on
 * the device's null stream and returns when the bytes are there.  The scratch (classes, word starts, chunk maps, the file
 * image) is kept per device, grow-only; vp_mseed_encode_release_scratch frees it -- the other release calls do not touch
 * it.  No counterpart of the kernels in the reference (ObsPy packs with libmseed on the host). */
typedef struct {
  int64_t start_us;      /* first sample, microseconds since 1970-01-01T00:00:00 UTC */
  double sample_rate;    /* Hz */
  int64_t first_sample;  /* where the trace begins in `samples`, in elements */
  int64_t nsamples;
  int32_t quality;       /* data quality indicator character: 'D', 'R', 'Q' or 'M' */
  char network[4], station[8], location[4], channel[4]; /* NUL terminated, as in vp_mseed_record */
} vp_mseed_trace;
enum { VP_MSEED_ENCODE_CHUNK = 2048 };  /* samples per chunk of the Steim packer: sizes around it take other paths */
enum { VP_MSEED_ENCODE_STAGES = 6 };    /* classify, chunk maps, compose, emit, pack, plain */
int vp_mseed_encode(int device_id, const void* samples, int samples_mem, int sample_kind, const vp_mseed_trace* traces,
                    int64_t n_traces, int reclen, int encoding, int big_endian, int b1001_mode, uint8_t* out_host,
                    size_t out_cap, size_t* out_bytes, int64_t* n_records, int64_t* bad_trace, int64_t* bad_sample);
/* The SEED sample-rate factor and multiplier of `rate` (host only): the smallest m in 1..32767 with rate * m an integer in
 * 1..32767 gives (rate * m, 1 if m == 1 else -m); else an integer period 1 / rate in 1..32767 gives (-1 / rate, 1); the pair
 * must give `rate` back exactly, anything else is VP_ERR_INVALID. */
int vp_mseed_rate_fields(double rate, int32_t* factor, int32_t* multiplier);
/* The 64-byte headers of the records of one trace (host only, no GPU, callable from any thread): record r holds
 * rec_count[r] samples from the trace's sample rec_first[r], and gets sequence number first_sequence + r (modulo 10^6).
 * headers: n_records * 64 bytes.  b1001_mode as above, decided over these records.  VP_ERR_INVALID as for vp_mseed_encode;
 * a rec_count beyond 65535 too. */
int vp_mseed_record_headers(const vp_mseed_trace* trace, const int64_t* rec_first, const int64_t* rec_count,
                            int64_t n_records, int64_t first_sequence, int reclen, int encoding, int big_endian,
                            int b1001_mode, uint8_t* headers);
/* Mean kernel time (ms, HIP events, after warm-up) of each stage of `iters` encodes of device-resident samples:
 * ms[VP_MSEED_ENCODE_STAGES] = classify, chunk maps, compose, emit, pack (Steim; 0 otherwise), plain (0 for Steim).  Bench only. */
int vp_mseed_encode_bench(int device_id, const void* samples_dev, int sample_kind, const vp_mseed_trace* traces,
                          int64_t n_traces, int reclen, int encoding, int big_endian, int iters, float* ms);
int vp_mseed_encode_release_scratch(int device_id, size_t* bytes_freed);

/* ---------------------------------------------------------------------------------------------
 * Sampling-rate conversion by an integer factor, on the device: what SeisBench's annotate() does to a trace whose rate
 * is an integer multiple of the model's -- trace.filter("lowpass", freq = new Nyquist, zerophase = True), then
 * trace.decimate(factor, no_filter = True) -- and volpick_amd/resample.py restates on the host with scipy:
 *
 *     f = sosfilt(sos, x);  g = sosfilt(sos, f[::-1])[::-1];  y = g[::factor]
 *
 * both passes from zero state, edge transients at both ends included.  in_dev: n samples in device memory, int32,
 * float32 or float64 (in_kind).  sos: HOST array of n_sections rows b0 b1 b2 a0 a1 a2 (scipy's layout, a0 == 1) in
 * double; 1 <= n_sections <= 4.  out_dev: out_len = ceil(n / factor) float32 samples in device memory.  State and the
 * intermediate f are float64 (f lives in a per-device scratch of 8 bytes per input sample); the only rounding to
 * float32 is the final store.  A NaN or Inf anywhere in the input makes every output sample NaN, as the whole-trace
 * recursion does (scipy keeps Inf only for an Inf within a few samples of the trace's end; here that is NaN too).
 *
 * The trace is filtered in pieces that start a warm-up ahead of themselves from zero state; the warm-up W is taken from
 * the largest pole radius r of `sos` so that r^W <= 2^-40.  VP_ERR_INVALID: factor < 2, n < 1, n_sections out of range,
 * out_len != ceil(n / factor), a0 != 1, an unstable or non-finite section.  VP_ERR_UNSUPPORTED: W exceeds the 1024
 * samples the kernel's tile has room for (4-corner Butterworth at 1 / factor of Nyquist: factor <= 40 fits).
 * Runs on the device's null stream and returns after the work is done, as vp_mseed_decode does; a caller whose input
 * was produced on a non-blocking stream synchronises that stream first.  Calls on one device are serialised.
 *
 * The scratch is kept per device, grow-only, between calls; vp_decimate_release_scratch frees it (bytes_freed may be
 * NULL) -- vp_mseed_release_scratch does not touch it.  vp_decimate_lowpass_bench: mean time in ms (HIP events on a
 * stream of its own, three untimed repetitions first) of `iters` repetitions of both passes (ms_total) and of the
 * forward pass alone (ms_forward, may be NULL): bench only. */
enum { VP_SAMPLES_FLOAT64 = 2 };
int vp_decimate_lowpass(int device_id, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                        int factor, float* out_dev, int64_t out_len);
int vp_decimate_release_scratch(int device_id, size_t* bytes_freed);
int vp_decimate_lowpass_bench(int device_id, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                              int factor, float* out_dev, int64_t out_len, int iters, float* ms_total, float* ms_forward);

/* ---------------------------------------------------------------------------------------------
 * Sampling-rate conversion by a non-integer ratio, on the device: what SeisBench's annotate() does to every other trace
 * -- trace.resample(model_rate, no_filter = True), ObsPy's Fourier method with a Hann window -- and
 * volpick_amd/resample.py:resample_fourier restates on the host with scipy:
 *
 *     X = rfft(x) * ifftshift(hann(n))[:n/2+1];  Y = interp(d_large_f * m, df * k, X);  y = irfft(Y) * num / n
 *
 * in_dev: n samples in device memory, int32, float32 or float64 (in_kind).  num, df and d_large_f are what the host
 * function forms, passed in so that both sides use the same float64 values: num = int(n / (rate_in / rate_out)),
 * df = 1.0 / (n * (1.0 / rate_in)), d_large_f = 1.0 / num * rate_out.  out_dev: out_len == num float32 samples in device
 * memory.  Both transforms are Bluestein chirp-z convolutions over power-of-two complex float64 FFTs of M >= 2 L - 1
 * points (L = n, then L = num), so n and num may be anything (primes included); the chirp phase is reduced in 64-bit
 * integers; the only rounding to float32 is the final store.  float32 input is widened and transformed in float64 (the
 * host path transforms float32 input in single precision, so it is the less accurate of the two).  A NaN or Inf anywhere
 * in the input makes every output sample NaN, as the host transform does.
 *
 * VP_ERR_INVALID: a null pointer, an unknown in_kind, n < 1, num < 1, out_len != num, a rate or frequency step that is
 * not finite and positive.  VP_ERR_UNSUPPORTED: max(n, num) needs an FFT beyond 2^27 points (2 max(n, num) - 1 > 2^27;
 * a 250 Hz component-day takes 2^26).  VP_ERR_NOMEM: the scratch cannot be allocated.  No partial result in any case.
 * Runs on the device's null stream and returns after the work is done, as vp_decimate_lowpass does.  Calls on one device
 * are serialised.
 *
 * The scratch (two FFT buffers of 16 M bytes, the half spectrum, a twiddle table) is kept per device, grow-only, between
 * calls; vp_resample_release_scratch frees it (bytes_freed may be NULL) -- the other release calls do not touch it.
 * vp_resample_fourier_bench: mean time in ms (HIP events on a stream of its own, three untimed repetitions first) of
 * `iters` repetitions of the whole conversion (ms_total) and of the forward transform alone (ms_forward, may be NULL):
 * bench only. */
int vp_resample_fourier(int device_id, const void* in_dev, int in_kind, int64_t n, double rate_in, double rate_out,
                        int64_t num, double df, double d_large_f, float* out_dev, int64_t out_len);
int vp_resample_release_scratch(int device_id, size_t* bytes_freed);
int vp_resample_fourier_bench(int device_id, const void* in_dev, int in_kind, int64_t n, double rate_in, double rate_out,
                              int64_t num, double df, double d_large_f, float* out_dev, int64_t out_len, int iters,
                              float* ms_total, float* ms_forward);

/* ---------------------------------------------------------------------------------------------
 * Filtering and detrending on the device: ObsPy's trace.filter(...) and trace.detrend(...), which
 * volpick_amd/signal.py restates on the host with scipy.
 *
 *     y = sosfilt(sos, x)                              zerophase == 0
 *     y = sosfilt(sos, sosfilt(sos, x)[::-1])[::-1]    zerophase != 0
 *
 * from zero state, edge transients included.  in_dev: n samples in device memory, int32, float32 or float64 (in_kind).
 * sos: HOST array of n_sections rows b0 b1 b2 a0 a1 a2 (scipy's layout, a0 == 1) in double; 1 <= n_sections <= 4, which
 * covers ObsPy's 4-corner low-pass and high-pass (2 sections) and band-pass and band-stop (4); a first-order section
 * (b2 == a2 == 0) is fine.  out_dev: n float32 samples in device memory; it must not overlap in_dev.  Coefficients,
 * state and the intermediate of the zero-phase form are float64; the only rounding to float32 is the final store, so
 * |y - scipy's float64 answer| <= 2^-24 |y| plus float64 noise (tests: 2^-22 max|x| on every sample).
 *
 * Scheme: the filter state z (2 doubles per section) is linear in itself, z <- A z + B x per sample, so a run of L samples
 * from state z0 ends in A^L z0 + (its end from zero state).  A pass is cut into tiles of 8192 samples and pieces of 32;
 * the host squares A into the table A^(32 2^k), k = 0..15, and three launches carry the state EXACTLY across every seam:
 * per tile, a scan of the pieces' zero-state ends to the tile's; one workgroup that scans the tiles' ends, 256 at a time,
 * to every tile's true start state; per tile, the scan again from that state and every piece run from its true start.
 * No pole radius is too close to 1 for it (unlike the warm-up of vp_decimate_lowpass).  Order between tiles comes from
 * the launch boundaries alone; no atomics: the same call gives the same bits twice.
 *
 * Non-finite input behaves as the whole-trace recursion does: one pass is right ahead of the first NaN and NaN from it on
 * (an Inf turns into NaN within the samples the recursion itself needs); a zero-phase call is NaN everywhere.
 *
 * VP_ERR_INVALID, out_dev untouched: a null pointer, an unknown in_kind, n < 0, n_sections outside 1..4, a0 != 1, a
 * non-finite coefficient, a section with a pole of radius >= 1, out_dev overlapping in_dev.  n == 0 does nothing.
 * VP_ERR_NOMEM: the scratch cannot be allocated.  Runs on the device's null stream and returns after the work is done, as
 * vp_decimate_lowpass does; calls on one device are serialised.
 *
 * The scratch (the table, 128 bytes per tile, 8 bytes per sample for a zero-phase call; a detrend's partial sums) is kept
 * per device, grow-only, between calls; vp_sos_filter_release_scratch frees it (bytes_freed may be NULL) -- the other
 * release calls do not touch it.  vp_sos_filter_bench: mean time in ms (HIP events on a stream of its own, three untimed
 * repetitions first) of `iters` repetitions of the whole filter (ms_total) and of one pass's carry launch alone
 * (ms_carry, may be NULL): bench only.
 *
 * vp_detrend: out = x minus its mean (VP_DETREND_DEMEAN, ObsPy's "demean" / "constant"), minus its least-squares line
 * (VP_DETREND_LINEAR, scipy.signal.detrend) or minus the line through its first and last sample
 * (VP_DETREND_SIMPLE: x[i] - (x[0] + i (x[n-1] - x[0]) / (n - 1)), ObsPy's default).  The sums are float64 in a fixed order
 * (per-workgroup partials, then one workgroup), the index centred on (n - 1) / 2 for the line; out_dev is float32 and must
 * not overlap in_dev.  VP_ERR_INVALID: as above, an unknown type, a line through fewer than two samples.  n == 0 with
 * VP_DETREND_DEMEAN does nothing. */
int vp_sos_filter(int device_id, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                  int zerophase, float* out_dev);
int vp_sos_filter_release_scratch(int device_id, size_t* bytes_freed);
int vp_sos_filter_bench(int device_id, const void* in_dev, int in_kind, int64_t n, const double* sos, int n_sections,
                        int zerophase, float* out_dev, int iters, float* ms_total, float* ms_carry);
enum { VP_DETREND_DEMEAN = 0, VP_DETREND_LINEAR = 1, VP_DETREND_SIMPLE = 2 };
int vp_detrend(int device_id, const void* in_dev, int in_kind, int64_t n, int type, float* out_dev);

/* ---------------------------------------------------------------------------------------------
 * PhaseNet training step (BASELINE config 5): what one
 * PhaseNetLit.training_step + Adam optimizer.step of the reference computes
 * (the reference's volpick/model/models.py:34-51 vector_cross_entropy, :160-164 training_step,
 * :177-185 torch.optim.Adam).  vp_train_create: fp32 throughout (what the reference trains in: no autocast).
 * vp_train_create_dtype(..., VP_TRAIN_BF16, ...): the activation and gradient rows of every layer (z, a, gz, ga -- all
 * of the step's HBM traffic but the weights) rest in memory as bfloat16, round-to-nearest-even on store; weights,
 * weight gradients, BatchNorm statistics, the loss and the Adam state stay fp32 and every product accumulates in
 * fp32 (BASELINE config 5's dtype).  Inputs, labels, predictions and everything vp_train_read returns are fp32 in
 * both modes; vp_train_tensor_read widens.
 *
 * vp_train_create uploads the flat weight blob (same order as vp_create; BatchNorm running
 * statistics included) and sizes the workspace for max_batch windows.  vp_train_step runs
 * forward in training mode (batch statistics; running statistics updated with momentum 0.1),
 * the loss -(1/B) sum_b sum_c mean_t y log(p + 1e-5), backward, and -- if update != 0 -- one Adam
 * step with learning rate lr (the caller owns the schedule, e.g. the reference's 500-step
 * warm-up, models.py:168-175).  x, y: (B, 3, 3001) fp32, host or device (mem).  *loss (may be
 * NULL; non-NULL synchronises) receives the batch loss.  vp_train_read copies out 0 = weights,
 * 1 = gradients of the last step, 2/3 = Adam first/second moments, 4 = EMA weights. */
typedef struct vp_trainer vp_trainer;
#define VP_TRAIN_FP32 0
#define VP_TRAIN_BF16 1
int vp_train_create(int device_id, int model_kind, const float* weights, size_t n_floats, int max_batch,
                    vp_trainer** out);
int vp_train_create_dtype(int device_id, int model_kind, const float* weights, size_t n_floats, int max_batch, int dtype,
                          vp_trainer** out);
int vp_train_dtype(const vp_trainer* t); /* VP_TRAIN_FP32 / VP_TRAIN_BF16 */
int vp_train_destroy(vp_trainer* t);
/* Adam's betas and eps, the BatchNorm momentum and the eps of log(p + eps) (defaults 0.9, 0.999, 1e-8, 0.1, 1e-5), in force
 * from the next vp_train_step.  VP_ERR_INVALID, with the previous five still in force, unless 0 <= beta1, beta2 < 1 (the
 * update divides by 1 - beta^t), adam_eps and loss_eps are finite and > 0, and 0 < bn_momentum <= 1; a NaN fails each of
 * these.  The update count t is the number of vp_train_step calls with update != 0: a step with update == 0 leaves the
 * weights, both moments, t and the EMA alone and still moves the BatchNorm running statistics. */
int vp_train_set_hyper(vp_trainer* t, float beta1, float beta2, float adam_eps, float bn_momentum, float loss_eps);
/* Optional exponential moving average of the weights after every update (the reference's EMA callback,
 * volpick/model/train.py:153-176: decay 0.999, every step); starts at the current weights. */
int vp_train_set_ema(vp_trainer* t, float decay);
int vp_train_step(vp_trainer* t, const float* x, const float* y, int mem, int B, float lr, int update, double* loss);
int vp_train_synchronize(vp_trainer* t);
/* The trainer runs on its own non-blocking stream (vp_train_stream).  A caller that hands vp_train_step DEVICE x / y
 * produced on another stream (a) makes the trainer's stream wait for them before the call (an event of its stream that
 * vp_train_stream waits for) and (b) calls this afterwards: `stream` (hipStream_t, NULL = legacy default stream) then
 * waits, on the device, for the point behind the step's last read of x / y -- so refilling or freeing them on `stream`
 * cannot overtake a queued step.  Host x / y are staged inside vp_train_step and need neither. */
int vp_train_wait_inputs_consumed(vp_trainer* t, void* stream);
/* The number (0 = this trainer's first vp_train_step) of the latest step whose reads of x / y are known to have completed,
 * -1 if none: a caller that keeps device batches alive for queued steps may drop those of steps <= the result.  No host
 * wait, nothing enters the trainer's stream (an event recorded there per step cost ~30 us of the step). */
long long vp_train_inputs_consumed_upto(vp_trainer* t);
long long vp_train_steps_enqueued(const vp_trainer* t);  /* the step a vp_train_step call just queued has the number (this - 1) */
int vp_train_read(vp_trainer* t, int which, float* out, size_t n_floats);
/* Replaces the whole flat blob (host pointer, the layout of vp_train_create: weights AND BatchNorm running statistics) once
 * the queued steps have finished.  Nothing else moves: the Adam moments, the update count t, the hyper-parameters and the
 * EMA stay what they were.  The next step therefore computes, bit for bit, what a new trainer created from the blob
 * computes for the same batch (loss, gradients, stored tensors, running statistics), and the next update continues Adam
 * from the old moments with t + 1.  A caller that wants a fresh optimiser creates a new trainer. */
int vp_train_write_weights(vp_trainer* t, const float* weights, size_t n_floats);
int vp_train_predictions(vp_trainer* t, float* out, int B);
/* Debug / parity tests: the z, a, gz, ga tensors of the last step as dense (B, C, L) arrays. */
int vp_train_tensor_count(const vp_trainer* t);
int vp_train_tensor_info(const vp_trainer* t, int index, const char** name, int* channels, int* length);
int vp_train_tensor_read(vp_trainer* t, int index, int B, float* out);
void* vp_train_stream(const vp_trainer* t);
int vp_train_launch_count(const vp_trainer* t); /* kernel launches the latest vp_train_step enqueued */

/* ---------------------------------------------------------------------------------------------
 * EQTransformer: training step of the three decoder stacks and their heads with the trunk frozen -- decoder_d with conv_d,
 * pick_decoders.{0,1} with pick_convs.{0,1}: 48 tensors, 145,731 floats.  What one EQTransformerLit.training_step + Adam
 * optimizer.step of the reference computes (volpick/model/models.py:538-549 shared_step, torch.nn.BCELoss per head,
 * torch.optim.Adam) when only those tensors require a gradient.  Everything is fp32; the loss value is the float64 one of
 * vp_bce_loss.  The decoders have no BatchNorm, dropout or recurrence, so the frozen trunk is the inference path: the
 * trainer builds a plan of its own from `weights` (the model's whole flat blob, host memory) and `cfg` (NULL: the
 * defaults) and runs, per step, the launches in front of the first decoder stage.  It holds no reference to any vp_handle.
 *
 * vp_eqt_dec_train_step: x (B, 3, 6000), already normalised (the forward pass of vp_forward with preprocess = 0); y
 * (B, 3, 6000) with the rows detection, P, S -- what vp_bank_make_batch_eqt writes for label_rows = {0, 1, 2}; both host or
 * both device (mem).  loss_weights: three doubles on the host (detection, P, S; the reference's 0.05, 0.40, 0.55).  Forward,
 * loss, backward and -- if update != 0 -- one Adam step at `lr` (torch's defaults: no weight decay; the caller owns the
 * schedule).  update == 0 leaves the weights, both moments and the update count alone.  *loss (may be NULL; non-NULL
 * synchronises) receives the batch loss.  Device x / y are read on the trainer's stream (vp_eqt_dec_train_stream): they must
 * be complete when the call is made and stay untouched until it has synchronised.
 * vp_eqt_dec_train_step_bank / _step_bank_aug: the batch of `rows` is generated as vp_bank_make_batch_eqt /
 * vp_bank_make_batch_eqt_aug generate it, straight into the trainer's buffers on its stream, then the step.
 * Refused before any launch: B outside [1, max_batch], a non-finite lr or loss weight, what the generation calls refuse
 * (VP_ERR_INVALID); a PhaseNet blob (VP_ERR_UNSUPPORTED).  The order of every sum is fixed and there are no atomics: two
 * trainers in the same state that take the same batches hold the same bits.
 *
 * vp_eqt_dec_train_read: 0 weights, 1 gradients of the last step, 2 / 3 Adam first / second moments: the
 * vp_eqt_dec_train_weight_count() floats of the 48 tensors in the flat blob's order (vp_eqt_dec_train_param_count / _name /
 * _size list them; host-only calls).  vp_eqt_dec_train_write_weights replaces those floats once the queued steps have
 * finished; the moments and the update count stay.  vp_eqt_dec_train_set_hyper: as vp_train_set_hyper refuses, for
 * beta1, beta2 and adam_eps.
 * vp_eqt_dec_train_tensor_*: the tensors of the last step, each a dense (sets, B, channels, length) block with sets = 3
 * decoders in the order detection, P, S: "decoder.in", "a0" .. "a6" (stage outputs after the ReLU), "logits", "gz_head"
 * (dLoss / dlogit), "ga0" .. "ga6", "gz0" .. "gz6" (gradient with respect to a stage's output after / before its ReLU);
 * "p" is the predictions, (1, B, 3, 6000).  B = the batch of the last step.
 * vp_eqt_dec_train_set_timing(t, 1) records an event between the step's phases; vp_eqt_dec_train_phase_ms then waits for
 * the last step and returns five times in ms: trunk, forward + heads + loss, input gradients, weight gradients, Adam.
 * One thread at a time per trainer. */
typedef struct vp_eqt_dec_trainer vp_eqt_dec_trainer;
int vp_eqt_dec_train_param_count(void);
const char* vp_eqt_dec_train_param_name(int index);
size_t vp_eqt_dec_train_param_size(int index);
size_t vp_eqt_dec_train_weight_count(void);
int vp_eqt_dec_train_create(int device_id, const float* weights, size_t n_floats, const vp_config* cfg, int max_batch,
                            vp_eqt_dec_trainer** out);
int vp_eqt_dec_train_destroy(vp_eqt_dec_trainer* t);
int vp_eqt_dec_train_set_hyper(vp_eqt_dec_trainer* t, float beta1, float beta2, float adam_eps);
int vp_eqt_dec_train_step(vp_eqt_dec_trainer* t, const float* x, const float* y, int mem, int B, const double* loss_weights,
                          float lr, int update, double* loss);
int vp_eqt_dec_train_synchronize(vp_eqt_dec_trainer* t);
int vp_eqt_dec_train_read(vp_eqt_dec_trainer* t, int which, float* out, size_t n_floats);
int vp_eqt_dec_train_write_weights(vp_eqt_dec_trainer* t, const float* weights, size_t n_floats);
int vp_eqt_dec_train_tensor_count(const vp_eqt_dec_trainer* t);
int vp_eqt_dec_train_tensor_info(const vp_eqt_dec_trainer* t, int index, const char** name, int* sets, int* channels,
                                 int* length);
int vp_eqt_dec_train_tensor_read(vp_eqt_dec_trainer* t, int index, int B, float* out);
void* vp_eqt_dec_train_stream(const vp_eqt_dec_trainer* t);
int vp_eqt_dec_train_launch_count(const vp_eqt_dec_trainer* t); /* kernel launches the latest step enqueued */
int vp_eqt_dec_train_set_timing(vp_eqt_dec_trainer* t, int on);
int vp_eqt_dec_train_phase_ms(vp_eqt_dec_trainer* t, float* ms);

/* A second training scope of the same trainer: VP_EQT_TRAIN_PICK_BRANCHES adds the two pick branches in front of the P and
 * S decoders -- pick_lstms.{0,1} (nn.LSTM(16, 16) over 47 steps) and pick_attentions.{0,1} (additive self-attention, 32
 * units, band of 3) -- to the trained tensors: 66 tensors, 152,261 floats, in the flat blob's order.  The bottleneck
 * ("decoder.in" set 0, the branches' input) and everything in front of it stay frozen; gradients into it are not formed.
 * The branches run their TRAINING forward in fp32: SeisBench's nn.Dropout(drop_rate) sits between the LSTM and its
 * attention, hd = h mask / (1 - drop_rate).  The mask element (branch, window index in the batch, channel, time step) is a
 * function of (seed, the trainer's count of steps, those four indices) through Philox4x32-10; the rule is stated in
 * volpick_amd/csrc/philox.h.  Every step advances the count, also one with update == 0: two steps never share a mask.
 * drop_rate == 0 keeps every element at scale 1: the step is then the derivative of the inference function.  The gradient of
 * pick_attentions.*.ba is identically zero (a constant of a score row cancels against the row's maximum); +0.0 is written.
 * vp_eqt_dec_train_create_scope: scope VP_EQT_TRAIN_DECODERS builds exactly the trainer of vp_eqt_dec_train_create (drop_rate
 * and seed are then unused, but drop_rate is checked all the same); refused with VP_ERR_INVALID, for either scope: another
 * scope, a drop_rate outside [0, 1) (NaN included), and what vp_eqt_dec_train_create refuses, under this entry's name.
 * Every per-handle entry above works on a handle of either scope with the handle's own sizes
 * (vp_eqt_dec_train_scope_weight_count(vp_eqt_dec_train_scope(t)) floats for _read / _write_weights).
 * Tensors of scope 1 besides those above, each (2 branches, B, channels, 47) unless said: "pick.x" (1, B, 16, 47: the
 * bottleneck), "pick.pre", "pick.act" (64 gate rows, torch's order i, f, g, o), "pick.c", "pick.h", "pick.mask" (0 / 1),
 * "pick.hd", "pick.v" (16), "pick.q", "pick.k" (32), "pick.e" (scores) and "pick.a" (47 x 47, row i, column j), "pick.argmax"
 * (1 row; the kept column of each row's maximum, as float); backward: "pick.gv" (stage 0's input gradient), "pick.gq",
 * "pick.gk" (32), "pick.ghd", "pick.gh", "pick.gc" (the cell gradient entering step t's backward, f_{t+1} dc_{t+1}),
 * "pick.gpre" (64).  vp_eqt_dec_train_pick_ms: with timing on, the three pick parts of the last step alone in ms -- forward,
 * adjoints (stage 0's input gradient, attention, dropout, LSTM), weight gradients -- which vp_eqt_dec_train_phase_ms counts
 * under its phases 1, 2 and 3. */
enum { VP_EQT_TRAIN_DECODERS = 0, VP_EQT_TRAIN_PICK_BRANCHES = 1 };
int vp_eqt_dec_train_create_scope(int device_id, const float* weights, size_t n_floats, const vp_config* cfg, int max_batch,
                                  int scope, float drop_rate, uint64_t seed, vp_eqt_dec_trainer** out);
int vp_eqt_dec_train_scope(const vp_eqt_dec_trainer* t);
int vp_eqt_dec_train_scope_param_count(int scope);
const char* vp_eqt_dec_train_scope_param_name(int scope, int index);
size_t vp_eqt_dec_train_scope_param_size(int scope, int index);
size_t vp_eqt_dec_train_scope_weight_count(int scope);
int vp_eqt_dec_train_pick_ms(vp_eqt_dec_trainer* t, float* ms);

/* ---------------------------------------------------------------------------------------------
 * Training batches generated on the GPU from a device-resident waveform bank: the window cut, Normalize and
 * ProbabilisticLabeller steps of the reference's augmentation block 1 (volpick/model/models.py:221-265).  The host plans
 * every random choice (volpick_amd/generate.py) and hands one vp_plan_row per window; the kernel has no RNG.
 *
 * vp_bank_create reserves n_traces traces holding n_floats_total floats in all.  vp_bank_write stores traces
 * [first_trace, first_trace + n_traces) -- in order: first_trace is the number of traces written so far -- from `data`,
 * their (3, trace_lengths[i]) fp32 arrays back to back, host or device (mem; a device source is read after every stream
 * of the device has drained), and their onsets: onsets[4 i .. 4 i + 3] = P, P, S, S in trace samples (float64, NaN = no
 * pick).  It may be called in chunks.  vp_bank_destroy synchronises the bank's device, then frees it.
 *
 * A plan row defines x[c][t] = bank[trace][c][start + t] where lo <= start + t < hi, else 0, for t in [0, T).
 * vp_bank_make_batch writes x and y, each (B, 3, T) fp32 on the bank's device, on `stream` (hipStream_t, NULL = legacy
 * default stream):
 *   x: per channel, minus its mean over the T samples, divided by max|x| + 1e-10 (norm = VP_NORM_PEAK) or by the
 *      population standard deviation (ddof 0) + 1e-10 (VP_NORM_STD);
 *   y: row label_rows[0] (P) and label_rows[1] (S): the maximum over the phase's onsets of exp(-(t - o)^2 / (2 sigma^2)),
 *      o = onset - start; row label_rows[2] (noise): clip(1 - P - S, 0, 1).
 * Every row and argument is checked on the host first (0 <= trace < traces written, 0 <= lo <= hi <= the trace's length,
 * 1 <= B, 1 <= T <= 6144, sigma > 0, label_rows a permutation of 0, 1, 2): VP_ERR_INVALID launches nothing and leaves x
 * and y untouched.  `rows` is host memory the caller may reuse as soon as the call returns.
 *
 * vp_train_step_bank is vp_train_step with x and y generated this way (T = 3001) into the trainer's own input buffers
 * on the trainer's stream: no upload and no wait on another stream.  The bank must live on the trainer's device and stay
 * alive until the step has run. */
typedef struct vp_bank vp_bank;
typedef struct {
  int32_t trace;
  int32_t reserved; /* 0 */
  int64_t start, lo, hi;
} vp_plan_row;
int vp_bank_create(int device_id, long long n_traces, long long n_floats_total, vp_bank** out);
int vp_bank_write(vp_bank* bank, long long first_trace, long long n_traces, const float* data, int mem,
                  const int64_t* trace_lengths, const double* onsets);
int vp_bank_destroy(vp_bank* bank);
/* vp_bank_read copies trace `trace` (written, or assembled on any stream: the bank's device is synchronised first) out as
 * its (3, length) fp32 array, to host or device memory (mem). */
int vp_bank_read(vp_bank* bank, long long trace, float* out, int mem);
/* vp_bank_assemble is vp_bank_write for traces that are still scattered over device-resident source arrays: it writes
 * traces [first_trace, first_trace + n_traces) -- in order, as vp_bank_write; trace_lengths and onsets as there -- from a
 * HOST table of pieces, in three launches on `stream` (hipStream_t, NULL = legacy default stream) for any number of
 * traces.  It is what the reference's conversion step computes per event file with ObsPy and numpy (its
 * volpick/data/convert.py:162 detrend("demean") and :26-70 stream_to_array), in float64:
 *
 *   a piece is one source trace's contribution to row (trace, component) of the bank.  src points at the first sample
 *   (device memory; int32, float32 or float64: kind, a VP_SAMPLES_* value) of the range the piece's own mean is taken
 *   over, mean_n samples: the source trace as it was when it was demeaned.  Of these, samples [keep_lo, keep_lo + keep_n)
 *   -- what the trims and the row's end leave -- go to row samples [dst, dst + keep_n) as x - mean(src[0 .. mean_n)).
 *   Pieces are grouped by row, rows ascending (trace, then component); within a row they stand in the order the
 *   reference writes them, and a row sample that several pieces cover takes the LAST of them (no racing stores: every
 *   row sample is written once, by the thread that has found its winner from the table).  Samples no piece covers
 *   are 0, a row without pieces is all 0.  Then the row's mean over all its samples, zeros included, is subtracted, and
 *   the result is rounded once to fp32:  bank = fp32((x - mean_piece) - mean_row).
 *
 * Sums are float64 in a fixed order that does not depend on the launch geometry: per piece and tile of
 * VP_ASSEMBLE_TILE samples one workgroup's partial sums (of x over the mean range, and of x and 1 over the samples the
 * piece wins), then one workgroup per row that adds its pieces' partials, forms the piece means and the row mean
 * (sum over pieces of [sum of won x - won count * piece mean] / row length); no atomics.  The same call gives the same
 * bits twice.  A source sample is read twice (sums, then the store), a bank sample written once.
 *
 * Everything is checked on the host first: first_trace is the number of traces written so far and the traces and their
 * floats fit the bank; every trace length >= 1; per piece first_trace <= trace < first_trace + n_traces, component in
 * 0..2, a known kind, a non-null src, mean_n >= 1, keep_n >= 1, 0 <= keep_lo and keep_lo + keep_n <= mean_n,
 * 0 <= dst and dst + keep_n <= the trace's length, rows ascending.  VP_ERR_INVALID launches nothing and leaves the bank
 * untouched.  `pieces` (n_pieces >= 0; may be NULL when 0), trace_lengths and onsets are host memory the caller may
 * reuse on return; the sources must stay alive and unchanged until the launches have run.  The call does not wait for
 * the device: the traces are there for work queued on `stream` behind it (another stream waits for `stream` first;
 * vp_bank_read and vp_bank_destroy synchronise the device themselves). */
#define VP_ASSEMBLE_TILE 4096
typedef struct {
  const void* src;
  int64_t mean_n;
  int64_t keep_lo, keep_n;
  int64_t dst;
  int32_t trace, component;
  int32_t kind;
  int32_t reserved; /* 0 */
} vp_assemble_piece;
int vp_bank_assemble(vp_bank* bank, long long first_trace, long long n_traces, const vp_assemble_piece* pieces,
                     long long n_pieces, const int64_t* trace_lengths, const double* onsets, void* stream);
int vp_bank_make_batch(vp_bank* bank, const vp_plan_row* rows, int B, int T, float sigma, int norm, const int* label_rows,
                       float* x, float* y, void* stream);
int vp_train_step_bank(vp_trainer* t, vp_bank* bank, const vp_plan_row* rows, int B, float sigma, int norm,
                       const int* label_rows, float lr, int update, double* loss);

/* Augmented windows: block 1 above, then volpick's stacking slots, AddGap and a second Normalize (the reference's
 * get_train_augmentations / get_val_augmentations with stack_data, volpick/model/models.py:345-440).  The host draws every
 * random choice and everything that follows from onsets alone (volpick_amd/generate.py, AugmentedPlanner); one
 * vp_aug_row per window is executed in this order:
 *   1. primary: x, y as vp_bank_make_batch writes them for `primary`;
 *   2. x[c][t] = 0 for t >= cut (cut = T: no truncation);
 *   3. per event entry with kind != VP_AUG_NONE, in order: the source s is `row` cut, demeaned, normalised and labelled
 *      as in step 1 (VP_AUG_BANK), or the primary window as it was after step 1 (VP_AUG_SELF, `row` all zero).
 *      VP_AUG_BANK only: every channel c whose current x[c] is all |x| <= 1e-8 is zeroed in s.  s[:, :zero_before] = 0;
 *      then x[c][t] += scale * s[c][t - shift] and y'[k][t] = y_s[k][t - shift] (0 where t - shift is outside [0, T));
 *      y = max(y, y') row by row, P and S divided by max(1, P + S), noise = 1 - P - S;
 *   4. per noise entry with kind == VP_AUG_BANK, in order: s as in step 3 (bank windows only, zero-channel rule), then
 *      x += s * max|x| * scale, max|x| over every channel of the current x;
 *   5. gauss > 0: x[c][t] += gauss * max(x) * n(noise_key, c, t), max(x) signed, n a standard normal from Philox4x32-10
 *      (key = noise_key, counter = (t, c, 0, 0)) through Box-Muller in float64: u_i = (w_{2i} | w_{2i+1} << 32) >> 11
 *      times 2^-53, n = sqrt(-2 log(1 - u_0)) cos(2 pi u_1);
 *   6. x[:, gap_lo:gap_hi] = 0; there y = 0 except the noise row, 1;
 *   7. x demeaned and normalised again with `norm` (float64 statistics, as in step 1).
 * Every field is checked on the host before any launch (VP_ERR_INVALID, outputs untouched): rows as for vp_plan_row,
 * kind in range, unused entries and reserved fields zero, 0 <= zero_before <= T, |shift| <= T (|shift| = T: the source
 * lies wholly outside the window, its labels still renormalise y), scales and gauss finite and >= 0, noise_key zero when
 * gauss is, 0 <= cut <= T, 0 <= gap_lo <= gap_hi <= T, and T <= 3072.  vp_train_step_bank_aug is vp_train_step_bank on such
 * rows. */
enum { VP_AUG_NONE = 0, VP_AUG_BANK = 1, VP_AUG_SELF = 2 };
typedef struct {
  vp_plan_row row;
  int32_t kind;        /* VP_AUG_* */
  int32_t zero_before;
  int32_t shift;
  float scale;
} vp_aug_event;
typedef struct {
  vp_plan_row row;
  int32_t kind;        /* VP_AUG_NONE or VP_AUG_BANK */
  float scale;
} vp_aug_noise;
typedef struct {
  vp_plan_row primary;
  vp_aug_event event[2];
  vp_aug_noise noise[2];
  uint64_t noise_key;
  float gauss;
  int32_t cut;
  int32_t gap_lo, gap_hi;
} vp_aug_row;
int vp_bank_make_batch_aug(vp_bank* bank, const vp_aug_row* rows, int B, int T, float sigma, int norm,
                           const int* label_rows, float* x, float* y, void* stream);
int vp_train_step_bank_aug(vp_trainer* t, vp_bank* bank, const vp_aug_row* rows, int B, float sigma, int norm,
                           const int* label_rows, float lr, int update, double* loss);

/* EQTransformer's batch: block 1 of the reference's EQTransformerLit (volpick/model/models.py:606-666) on vp_plan_row rows,
 * 1 <= T <= 6144.  vp_bank_make_batch_eqt writes x and y as vp_bank_make_batch does, with these rows of y:
 *   label_rows[1] (P) and label_rows[2] (S): as there, to the bit (ProbabilisticLabeller with noise_column=False: no noise
 *      row and no rescaling);
 *   label_rows[0] (detection): SeisBench's DetectionLabeller.  With p and s the earliest finite P and S onset relative to
 *      the window (float64), the row is 1 on the samples [max(int(p), 0), max(int(s + 1.4 (s - p)), 0)) that lie in the
 *      window and 0 elsewhere; all 0 when the trace has no finite P or no finite S onset, or s < p.  int() truncates toward
 *      zero; the product is rounded before the sum (no fused multiply-add), as Python rounds them.
 *      det_fixed_window >= 0 (samples; the reference's detection_fixed_window): s = p + det_fixed_window and the factor is
 *      0, S is not read.  Negative: the rule above.
 * x equals what vp_bank_make_batch writes for the same rows, to the bit.  Checked as vp_bank_make_batch checks, and
 * det_fixed_window negative or finite (VP_ERR_INVALID launches nothing and leaves x and y untouched). */
int vp_bank_make_batch_eqt(vp_bank* bank, const vp_plan_row* rows, int B, int T, float sigma, int norm, const int* label_rows,
                           float det_fixed_window, float* x, float* y, void* stream);

/* EQTransformer's augmented windows: the block 1 above, then the stacking slots, AddGap on y and detections and the second
 * Normalize of the reference's EQTransformerLit (get_train_augmentations / get_val_augmentations with stack_data,
 * volpick/model/models.py:668-844).  The records are the vp_aug_row of vp_bank_make_batch_aug, planned with EQTransformer's
 * windows (volpick_amd/generate.py, AugmentedPlanner with its event_* arguments); y has the rows label_rows[0] (detection
 * D), label_rows[1] (P) and label_rows[2] (S), no noise row.  One record per window is executed in this order:
 *   1. primary: x, P, S and D as vp_bank_make_batch_eqt writes them for `primary`;
 *   2. x[c][t] = 0 for t >= cut (cut = T: no truncation);
 *   3. per event entry with kind != VP_AUG_NONE, in order: the source s is `row` cut, demeaned and normalised as in step 1,
 *      with its own P_s, S_s and detection box D_s from the row's window-relative onsets (VP_AUG_BANK), or the primary
 *      window with its labels as they were after step 1 (VP_AUG_SELF, `row` all zero).  VP_AUG_BANK only: every channel c
 *      whose current x[c] is all |x| <= 1e-8 is zeroed in s.  s[:, :zero_before] = 0; then x[c][t] += scale * s[c][t - shift],
 *      P[t] = max(P[t], P_s[t - shift]) and S likewise -- noise_label = False: no division by max(1, P + S) -- and
 *      D[t] = max(D[t], D_s[t - shift]) ONLY WHEN shift != 0: the reference's shift of the detection row has no branch for
 *      an unshifted source, whose detection is therefore dropped while its waveform and its P and S are merged.  A position
 *      t - shift outside [0, T) contributes 0;
 *   4. noise entries and 5. Gaussian noise: as steps 4 and 5 of vp_bank_make_batch_aug (the labels are untouched; the same
 *      Philox key and counter);
 *   6. x = P = S = D = 0 on [gap_lo, gap_hi): no row is set to 1;
 *   7. x demeaned and normalised again with `norm` (float64 statistics, one rounding to fp32).
 * Checked on the host as vp_bank_make_batch_aug checks, field for field, with 1 <= T <= 6144, and det_fixed_window negative
 * or finite: VP_ERR_INVALID launches nothing and leaves x and y untouched.  vp_validate_eqt_bank_aug (below) is
 * vp_validate_eqt_bank on such records. */
int vp_bank_make_batch_eqt_aug(vp_bank* bank, const vp_aug_row* rows, int B, int T, float sigma, int norm,
                               const int* label_rows, float det_fixed_window, float* x, float* y, void* stream);
/* The decoder trainer's step (above) on a batch generated by the two calls above into its own buffers. */
int vp_eqt_dec_train_step_bank(vp_eqt_dec_trainer* t, vp_bank* bank, const vp_plan_row* rows, int B, float sigma, int norm,
                               const int* label_rows, float det_fixed_window, const double* loss_weights, float lr, int update,
                               double* loss);
int vp_eqt_dec_train_step_bank_aug(vp_eqt_dec_trainer* t, vp_bank* bank, const vp_aug_row* rows, int B, float sigma, int norm,
                                   const int* label_rows, float det_fixed_window, const double* loss_weights, float lr,
                                   int update, double* loss);

/* ---------------------------------------------------------------------------------------------
 * Validation loss on the device: the reference's vector_cross_entropy (volpick/model/models.py:34-51) of predictions
 * that never leave the GPU, in float64, and the validation half of its training loop (validation_step, :171-174) on
 * batches generated from a waveform bank.
 *
 * vp_vce_loss reads p and y, dense (B, C, T) fp32 on device `device_id`, and writes on `stream` (hipStream_t, NULL =
 * legacy default stream), without waiting for it:
 *   per_window_dev[b] = -(1/T) sum_c sum_t y[b][c][t] * log((double)p[b][c][t] + eps)     (B doubles, may be NULL)
 *   batch_dev[0]      = (1/B) sum_b per_window_dev[b]                                      (1 double, may be NULL)
 * Every operation is a float64 one (eps is a double: 1e-5, not (double)1e-5f).  The order of every sum is fixed and there
 * are no atomics: the same arrays at the same addresses give the same bits (the order depends on the addresses mod 16 only).
 * NaN and Inf propagate as IEEE arithmetic takes them -- that window's value and the batch loss become NaN -- and are no
 * error.  With per_window_dev NULL the batch loss is the same number, computed by one workgroup: slow, for callers with
 * nowhere to put B doubles.  Checked on the host before any launch (VP_ERR_INVALID, outputs untouched): B >= 1,
 * 1 <= C <= 8, T >= 1, eps > 0, p and y not NULL.
 *
 * A validation pass on a PhaseNet handle; an EQTransformer handle gets VP_ERR_UNSUPPORTED, its loss has other labels (vp_validate_eqt_*):
 *   vp_validate_begin(h)        opens a pass: no batches yet.
 *   vp_validate_bank(h, ...)    enqueues one batch on the handle's stream and returns: rows cut, normalised and labelled as
 *                               vp_bank_make_batch does (T = vp_in_samples(h)) into scratch of the handle; the forward pass
 *                               on it as vp_forward(preprocess = 0) runs it, in chunks of max_batch windows; the loss of all
 *                               B windows (the batch value is their mean, not a mean of chunk means), appended with the B
 *                               window values to device arrays of the handle.  pred_out_dev, when not NULL, receives the
 *                               (B, 3, T) predictions (device memory no other stream is using).  Any B >= 1.  Rows and
 *                               arguments are checked as for vp_bank_make_batch, and eps > 0, before anything is enqueued.
 *   vp_validate_bank_aug        the same on vp_aug_row rows (vp_bank_make_batch_aug).
 *   vp_validate_end(h, ...)     waits for the stream -- the pass's only host wait in the steady state -- and copies out up
 *                               to `cap` batch losses and `cap_windows` window values, in the order enqueued; *n_batches and
 *                               *n_windows are how many the pass holds.  Closes the pass.
 * The host does wait inside a pass when a batch is larger than any before it on this handle, or a result array grows
 * (both reallocate), and when eight batches are in flight: a slot of the row staging ring is reused only behind the event
 * of the launch that read it.  `rows` may be reused as soon as the call returns.  The bank must live on the handle's
 * device and stay alive until vp_validate_end.  One thread at a time per handle, as for every call on a vp_handle; the
 * results of a pass do not depend on what ran before it (bit for bit). */
int vp_vce_loss(int device_id, const float* p_dev, const float* y_dev, int B, int C, int T, double eps,
                double* per_window_dev, double* batch_dev, void* stream);
int vp_validate_begin(vp_handle* h);
int vp_validate_bank(vp_handle* h, vp_bank* bank, const vp_plan_row* rows, int B, float sigma, int norm,
                     const int* label_rows, double eps, float* pred_out_dev);
int vp_validate_bank_aug(vp_handle* h, vp_bank* bank, const vp_aug_row* rows, int B, float sigma, int norm,
                         const int* label_rows, double eps, float* pred_out_dev);
int vp_validate_end(vp_handle* h, double* batch_losses, long long cap, long long* n_batches, double* per_window,
                    long long cap_windows, long long* n_windows);

/* ---------------------------------------------------------------------------------------------
 * EQTransformer's validation loss on the device: the weighted binary cross entropy of the reference's
 * EQTransformerLit.shared_step (volpick/model/models.py:538-549; torch.nn.BCELoss, mean reduction, once per head), in
 * float64, and a validation pass over a bank that computes it on the batch of vp_bank_make_batch_eqt.
 *
 * vp_bce_loss reads p and y, dense (B, C, T) fp32 on device `device_id`, and `weights`, C doubles on the HOST (read
 * before the call returns), and writes on `stream` (hipStream_t, NULL = legacy default stream), without waiting for it:
 *   term                = -( y max(log p, -100) + (1 - y) max(log(1 - p), -100) ),  p and y widened to double first
 *   head_dev[b * C + c] = (1/T) sum_t term of row c, unweighted                        (B * C doubles, may be NULL)
 *   per_window_dev[b]   = sum_c weights[c] * head[b][c]                                (B doubles, may be NULL)
 *   batch_dev[0]        = (1/B) sum_b per_window[b]                                    (1 double, may be NULL)
 * Every window has T samples, so batch_dev[0] = sum_c weights[c] * BCELoss(p[:, c], y[:, c]).  The clamp is torch's and
 * keeps a NaN; NaN, Inf and p outside [0, 1] propagate as IEEE arithmetic takes them and are no error.  Both logarithms are
 * taken of every element.  The order of every sum is fixed and there are no atomics: the same arrays at the same addresses
 * give the same bits (the order depends on the addresses mod 16 only).  With per_window_dev NULL the batch loss is the
 * same number, computed by one workgroup: slow.  Checked on the host before any launch (VP_ERR_INVALID, outputs
 * untouched): B >= 1, 1 <= C <= 8, T >= 1, p, y and weights not NULL, the weights finite.
 *
 * A validation pass on an EQTransformer handle; a PhaseNet handle gets VP_ERR_UNSUPPORTED (its pass is vp_validate_*):
 *   vp_validate_eqt_begin(h)       opens a pass: no batches yet.
 *   vp_validate_eqt_bank(h, ...)   enqueues one batch on the handle's stream and returns: rows cut, normalised and labelled
 *                                  as vp_bank_make_batch_eqt does (T = vp_in_samples(h) = 6000; label_rows = the rows of
 *                                  detection, P and S in the model's output: 0, 1, 2) into scratch of the handle; the
 *                                  forward pass as vp_forward(preprocess = 0) runs it, in chunks of max_batch windows; then
 *                                  vp_bce_loss of all B windows with weights[0..2] = the weights of detection, P and S
 *                                  (the reference's loss_weights: 0.05, 0.40, 0.55), appended to device arrays of the
 *                                  handle.  pred_out_dev, when not NULL, receives the (B, 3, T) predictions.  Any B >= 1.
 *                                  Everything is checked before anything is enqueued; a refused call appends nothing.
 *   vp_validate_eqt_bank_aug       the same on vp_aug_row records, generated as vp_bank_make_batch_eqt_aug does; it appends
 *                                  to the same open pass, and batches of either kind may alternate within one pass.
 *   vp_validate_eqt_end(h, ...)    waits for the stream -- the pass's only host wait in the steady state -- and copies out
 *                                  up to `cap` batch losses, `cap_windows` window values (per_window, may be NULL) and
 *                                  3 * `cap_windows` head values (heads, [window][row of y], may be NULL), in the order
 *                                  enqueued; *n_batches and *n_windows are how many the pass holds.  Closes the pass.
 * The host waits inside a pass where vp_validate_bank does.  A pass may be open beside a prediction or sweep pass of the
 * same handle; the results of a pass do not depend on what ran before it (bit for bit). */
int vp_bce_loss(int device_id, const float* p_dev, const float* y_dev, int B, int C, int T, const double* weights,
                double* head_dev, double* per_window_dev, double* batch_dev, void* stream);
int vp_validate_eqt_begin(vp_handle* h);
int vp_validate_eqt_bank(vp_handle* h, vp_bank* bank, const vp_plan_row* rows, int B, float sigma, int norm,
                         const int* label_rows, float det_fixed_window, const double* weights, float* pred_out_dev);
int vp_validate_eqt_bank_aug(vp_handle* h, vp_bank* bank, const vp_aug_row* rows, int B, float sigma, int norm,
                             const int* label_rows, float det_fixed_window, const double* weights, float* pred_out_dev);
int vp_validate_eqt_end(vp_handle* h, double* batch_losses, long long cap, long long* n_batches, double* per_window,
                        double* heads, long long cap_windows, long long* n_windows);

/* ---------------------------------------------------------------------------------------------
 * Pick-benchmark tasks 1-3: the per-window scores of the reference's predict_step (volpick/model/models.py:454-480 for
 * PhaseNet, :881-906 for EQTransformer; driven by volpick/model/eval_taks123.py:20-166), reduced on the device.
 *
 * For window b and its border [lo[b], hi[b]) (lo = hi = NULL: [0, T), T = vp_in_samples(h)) one vp_predict_record:
 *   det     VP_DET_ONE_MINUS_NOISE (PhaseNet; det_row is the noise row): max_t of the fp32 difference 1 - noise[t];
 *           VP_DET_ROW (EQTransformer; det_row is the detection trace): max_t det[t];
 *   p_max, s_max   the maxima of rows p_row and s_row inside the border;
 *   p_arg, s_arg   their positions relative to lo[b].
 * Maximum and argmax are torch's on the CPU: the lowest index among equal maxima; a NaN is above every number and the
 * first NaN wins, so a NaN in a row makes that row's maximum NaN.  The maximum is the value AT that index: -0 and +0 compare
 * equal, so a maximum of zero carries the sign of the first zero (torch's vectorised max may return either zero; nothing
 * else differs from it, bit for bit).  No atomics: the same input gives the same bits.
 * score_p_or_s of the reference is p_max / s_max; the library does not divide.  The caller forms the quotient on the host
 * in float32 (correctly rounded, x / 0 = inf, 0 / 0 = NaN), as volpick_amd/evaluate.py does.
 *
 * vp_predict_windows reduces prob, (B, n_rows, T) fp32 in host or device memory (prob_mem), into out[0 .. B) (host) and
 * returns when that is done: the loop of predict_step.  Checked on the host before any launch (VP_ERR_INVALID, `out`
 * untouched): null h / prob / out, lo without hi or hi without lo, B < 1, n_rows outside [3, 64], a row outside
 * [0, n_rows) or two rows equal, an unknown det_mode, a border with lo < 0, hi > T or hi <= lo (torch raises on the empty
 * slice; an empty border is an error here, never a zero).
 *
 * A pass over a waveform bank, for PhaseNet and EQTransformer handles alike, shaped like vp_validate_*:
 *   vp_predict_begin(h)        opens a pass: no windows yet.
 *   vp_predict_bank(h, ...)    enqueues one batch on the handle's stream and returns: the B rows cut, demeaned and
 *                              normalised exactly as vp_bank_make_batch does with `norm` (a kernel of its own that leaves
 *                              the label work out) into scratch of the handle; the forward pass on it as
 *                              vp_forward(preprocess = 0) runs it, in chunks of max_batch windows; the reduction above
 *                              on rows det_row / p_row / s_row of the three outputs, with the handle's own rule
 *                              (PhaseNet: VP_DET_ONE_MINUS_NOISE, det_row the noise row; EQTransformer: VP_DET_ROW,
 *                              rows 0 / 1 / 2); the B records appended to a device array of the handle.  pred_out_dev,
 *                              when not NULL, receives
 *                              the (B, 3, T) probabilities the records were reduced from (device memory no other stream
 *                              is using).  Any B >= 1.  Rows are checked as for vp_bank_make_batch and borders as above
 *                              before anything is enqueued.
 *   vp_predict_end(h, ...)     waits for the stream -- the pass's only host wait in the steady state -- and copies out up
 *                              to `cap` records in the order enqueued; *n_windows is how many the pass holds.  Closes it.
 * The host waits inside a pass where vp_validate_bank does (a larger batch than before, a growing result array, eight
 * batches in flight).  `rows`, `lo` and `hi` may be reused as soon as the call returns.  The bank must live on the handle's
 * device and stay alive until vp_predict_end.  One thread at a time per handle; the results of a pass do not depend on
 * what ran before it (bit for bit).  A validation pass and a prediction pass of one handle may be open together. */
enum { VP_DET_ONE_MINUS_NOISE = 0, VP_DET_ROW = 1 };
typedef struct {
  float det, p_max, s_max;
  int32_t p_arg, s_arg;
} vp_predict_record;
int vp_predict_windows(vp_handle* h, const float* prob, int prob_mem, int B, int n_rows, int det_row, int p_row, int s_row,
                       int det_mode, const int32_t* lo, const int32_t* hi, vp_predict_record* out);
int vp_predict_begin(vp_handle* h);
int vp_predict_bank(vp_handle* h, vp_bank* bank, const vp_plan_row* rows, const int32_t* lo, const int32_t* hi, int B,
                    int norm, int det_row, int p_row, int s_row, float* pred_out_dev);
int vp_predict_end(vp_handle* h, vp_predict_record* out, long long cap, long long* n_windows);

/* ---------------------------------------------------------------------------------------------
 * Pick-benchmark task 0: the threshold sweep of the reference's eval_task0 (volpick/model/eval_taks0.py:370-825; its
 * evaluate(), :20-200, runs the model once per threshold), every threshold from ONE set of probabilities on the device.
 *
 * For window b, its border [lo[b], hi[b]) (lo = hi = NULL: [0, T), T = vp_in_samples(h)), phase ph (0: row p_row, 1: row
 * s_row) and threshold pair j of NT, with x = prob[b][row][lo[b] .. hi[b]):
 *   count[(b * 2 + ph) * NT + j]             the triggers of ObsPy's trigger_onset(x, thr_on[j], thr_off[j]): one per run of
 *                                            consecutive samples > thr_off[j] that holds a sample > thr_on[j].  A run is cut
 *                                            at the border on both sides.  The count may exceed K.
 *   peak[((b * 2 + ph) * NT + j) * K + i]    trigger i < min(count, K), in sample order: the argmax of the span [first
 *                                            sample > thr_on[j] of the run, run end], relative to lo[b]; the lowest index
 *                                            among equal maxima.  The first K triggers are kept; slots i >= count hold -1.
 *   value[the same index]                    the maximum at peak; slots i >= count hold 0.  value may be NULL: nothing is
 *                                            computed into or copied out of it (the reference never saves the scores).
 * Thresholds are fp32 and every comparison is a strict fp32 `>`, vp_pick_windows' contract: a sample equal to a threshold
 * is below it, and a NaN ends a run and is never a maximum.  The reference calls this with thr_off = thr_on / 2.
 * thr_off[j] > thr_on[j] -- the corner vp_pick_host resolves the way ObsPy's loop happens to -- is REFUSED here.
 * Slots are numbered by counts and an exclusive scan in sample order, without atomics: entries ascend and the same input
 * gives the same bits.  One launch covers both phases and all NT thresholds and reads each border once.
 *
 * vp_sweep_windows sweeps prob, (B, n_rows, T) fp32 in host or device memory (prob_mem), into the host arrays count
 * [B][2][NT], peak [B][2][NT][K] and value (the same shape, or NULL) and returns when that is done.  Checked on the host
 * before anything is enqueued (VP_ERR_INVALID, the outputs untouched): null h / prob / thr_on / thr_off / count / peak, lo
 * without hi or hi without lo, a border with lo < 0, hi > T or hi <= lo, B < 1, NT outside [1, 32], K outside [1, 64],
 * n_rows outside [2, 64], a row outside [0, n_rows), p_row == s_row, a threshold that is not finite, thr_off[j] >
 * thr_on[j], and T above VP_SWEEP_MAX_T, the border the kernel's LDS row holds.
 *
 * A pass over a waveform bank, shaped like vp_predict_*:
 *   vp_sweep_begin(h, ...)    opens a pass with its NT threshold pairs, K and whether values are kept (keep_values != 0):
 *                             fixed for the pass, so that its results have one stride.  Checked as above.
 *   vp_sweep_bank(h, ...)     enqueues one batch on the handle's stream and returns: the B rows cut and normalised and
 *                             the forward pass run in chunks of max_batch exactly as vp_predict_bank does, then ONE sweep
 *                             launch on rows p_row / s_row; the results appended to device arrays of the handle.
 *                             pred_out_dev, when not NULL, receives the (B, 3, T) probabilities that were swept.  Any
 *                             B >= 1.  Rows are checked as for vp_bank_make_batch, the rest as above, before anything is
 *                             enqueued; a refused batch leaves the pass as it was.
 *   vp_sweep_end(h, ...)      waits for the stream -- the pass's only host wait in the steady state -- and copies out the
 *                             results of up to cap_windows windows in the order enqueued: count [n][2][NT], peak
 *                             [n][2][NT][K] and, when not NULL (the pass must have kept them), value.  *n_windows is how
 *                             many the pass holds.  Closes it.
 * The host waits inside a pass where vp_predict_bank does.  `rows`, `lo`, `hi` and the thresholds may be reused as soon as
 * the call returns.  The bank must live on the handle's device and stay alive until vp_sweep_end.  One thread at a time per
 * handle; the results of a pass do not depend on what ran before it (bit for bit).  A sweep pass may be open beside a
 * prediction pass and a validation pass of the same handle: each has its own scratch and results. */
#define VP_SWEEP_MAX_T 6400
int vp_sweep_windows(vp_handle* h, const float* prob, int prob_mem, int B, int n_rows, int p_row, int s_row, const int32_t* lo,
                     const int32_t* hi, const float* thr_on, const float* thr_off, int NT, int K, int32_t* count,
                     int32_t* peak, float* value);
int vp_sweep_begin(vp_handle* h, const float* thr_on, const float* thr_off, int NT, int K, int keep_values);
int vp_sweep_bank(vp_handle* h, vp_bank* bank, const vp_plan_row* rows, const int32_t* lo, const int32_t* hi, int B, int norm,
                  int p_row, int s_row, float* pred_out_dev);
int vp_sweep_end(vp_handle* h, int32_t* count, int32_t* peak, float* value, long long cap_windows, long long* n_windows);

/* ---------------------------------------------------------------------------------------------
 * Frequency index and signal-to-noise ratio of picks and bank traces, on the device: the trace_frequency_index,
 * trace_snr_db and trace_mean_snr_db columns the reference stores with every trace it writes (volpick/data/utils.py
 * freqency_index, calculate_snr; volpick/data/convert.py:222-270).  One vp_attr_row per pick or trace, planned on the
 * host (volpick_amd/attributes.py, plan_rows) from lengths and onsets alone; the rule is restated in
 * tests/attributes_f64.py.  Per row, in float64:
 *
 *   frequency index of component c: X = DFT of x[c][fi_start : fi_start + fi_n] times the symmetric Hann window, at bins
 *     [lo_first, lo_first + lo_count) and [hi_first, hi_first + hi_count) only; log10(mean |X| high / mean |X| low).
 *     NaN where a band is empty (a count of 0), where fi_n = 0 (no reference sample), where the window holds a NaN, and
 *     for a component whose sum |diff| over the WHOLE trace is <= 1e-9 (a dead channel).  The row's index is the mean of
 *     the components that are not NaN, NaN if none.
 *   percentile of a window of m samples (noise, signal): the values of rank `lo` and `up` of |x| (0-based, ascending),
 *     a + (b - a) g, or b - (b - a) (1 - g) where g >= 0.5 -- numpy's linear method, bit for bit where the host plans
 *     h = (m - 1) 0.95, lo = floor(h), up = min(lo + 1, m - 1), g = h - lo.  NaN if the window holds a NaN or m = 0.
 *   snr_db of a component: 20 log10(signal / noise), NaN where either percentile is <= 1e-8 (np.isclose(v, 0)); their
 *     mean over the components that are not NaN, NaN if none.
 *   VP_ATTR_DEMEAN: before all of the above, each component has its mean over the span from the row's earliest window
 *     start to its latest window end subtracted (raw counts carry an offset).
 *
 * out: n_rows x 14 float64, device or host memory (the call finds out): fi[3], fi_trace, noise_p95[3], signal_p95[3],
 * snr_db[3], snr_mean.  Deterministic: no atomics, every sum in a fixed order.  vp_attributes reads one (3, n_samples)
 * fp32 array on the device (every row's trace is 0); vp_bank_attributes reads the bank's traces (a row's `trace` indexes
 * the bank).  Both run the same kernel on `stream` (hipStream_t, NULL = legacy default stream) and return after the work
 * is done; `rows` is host memory.  Calls on one device are serialised.
 *
 * Every row is checked on the host first (VP_ERR_INVALID, nothing launched, out untouched): trace in range, windows
 * inside the trace and of at most 2048 samples, bins below fi_n / 2, 0 <= lo <= up <= lo + 1 < m, 0 <= g <= 1, unknown
 * flags.  VP_ERR_NOMEM: the scratch (staged rows, per-trace sums) cannot be allocated. */
#define VP_ATTR_DEMEAN 1
#define VP_ATTR_MAX_WINDOW 2048
#define VP_ATTR_OUT 14
typedef struct {
  int32_t trace;
  int32_t flags;                                /* VP_ATTR_DEMEAN */
  int64_t fi_start, noise_start, signal_start;  /* first sample of each window */
  int32_t fi_n, noise_n, signal_n;              /* their lengths; 0 = absent */
  int32_t lo_first, lo_count, hi_first, hi_count;
  int32_t noise_lo, noise_up, signal_lo, signal_up;
  int32_t reserved;                             /* 0 */
  double noise_g, signal_g;
} vp_attr_row;
int vp_attributes(int device_id, const float* data, int64_t n_samples, const vp_attr_row* rows, int n_rows, double* out,
                  void* stream);
int vp_bank_attributes(vp_bank* bank, const vp_attr_row* rows, int n_rows, double* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spectrograms on the device: the numbers of the reference's spectrogram() (volpick/data/utils.py:1251-1440) up to the point
 * where it starts to draw, i.e. matplotlib.mlab.specgram(data - data.mean(), Fs, NFFT, pad_to, noverlap) without bin 0, then
 * sqrt or 10 log10.  The host plans nfft, pad and hop from the sampling rate (volpick_amd/spectrogram.py, plan); the rule is
 * restated in tests/spectrogram_f64.py.  Per series, in float64:
 *
 *   x = data - mean(data), the mean over the WHOLE series (all n samples, whatever the frame range);
 *   frame j = x[j hop : j hop + nfft] times np.hanning(nfft), zero-padded to pad;  X = its DFT;
 *   P[k] = |X[k]|^2 / samp_rate / sum(w^2) for k = 1 .. pad / 2, doubled for every k but pad / 2;
 *   out = sqrt(P) (dbscale == 0) or 10 log10(P) (dbscale == 1), rounded once to float32.
 *
 * in_dev: n_series series of n samples each, series i at in_dev + i * series_stride samples, int32, float32 or float64
 * (in_kind): a (3, N) block or an (M, 3, L) tensor in one launch.  A series has (n - (nfft - hop)) / hop frames; the call
 * writes frames [first_frame, first_frame + n_frames) into out_dev, (n_series, pad / 2, n_frames) float32 in device memory,
 * frequency-major as the reference's specgram[f, t] (no flipud).  A frame range equals the same columns of the full result
 * bit for bit, so a day can be produced in pieces.  A NaN or Inf anywhere in a series makes that series' whole output NaN
 * (the reference's mean is non-finite then); a frame of exact zeros gives 0, or -inf with dbscale.  Deterministic: no
 * atomics, every sum in a fixed order.  For float32 input the reference's mean accumulates in float32; this one does not.
 *
 * Every argument is checked on the host before any launch; a refusal leaves out_dev untouched.  VP_ERR_INVALID: a null
 * pointer, an unknown in_kind, n_series < 1, n < nfft, hop < 1 or hop > nfft, nfft or pad not a power of two or pad < nfft,
 * a frame range outside [0, (n - (nfft - hop)) / hop], series_stride < n, a samp_rate that is not finite and positive,
 * dbscale other than 0 or 1.  VP_ERR_UNSUPPORTED: beyond nfft 32..512, pad / nfft <= 16, pad <= 4096, 65535 series of 2^40
 * samples.  VP_ERR_NOMEM: the scratch cannot be allocated.  n_frames == 0 is a valid call that writes nothing.
 *
 * Runs on `stream` (hipStream_t, NULL = legacy default stream) and returns after the work is done.  Calls on one device are
 * serialised.  A workgroup owns min(VP_SPECTROGRAM_TILE_FRAMES, 4096 / nfft) consecutive frames.  The scratch (the series'
 * means, the mean pass's partial sums, the window and root tables) is kept per device, grow-only, between calls;
 * vp_spectrogram_release_scratch frees it (bytes_freed may be NULL) -- the other release calls do not touch it.
 * vp_spectrogram_bench: mean time in ms (HIP events on a stream of its own, two untimed repetitions first) of `iters`
 * repetitions of the whole call (ms_total) and of the frame kernel alone (ms_frames, may be NULL): bench only. */
#define VP_SPECTROGRAM_TILE_FRAMES 32
int vp_spectrogram(int device_id, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n,
                   double samp_rate, int nfft, int pad, int hop, int dbscale, int64_t first_frame, int64_t n_frames,
                   float* out_dev, void* stream);
int vp_spectrogram_release_scratch(int device_id, size_t* bytes_freed);
int vp_spectrogram_bench(int device_id, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n,
                         double samp_rate, int nfft, int pad, int hop, int dbscale, int64_t first_frame, int64_t n_frames,
                         float* out_dev, int iters, float* ms_total, float* ms_frames);

/* ---------------------------------------------------------------------------------------------
 * STA/LTA characteristic functions of device-resident series and the triggers cut from them: ObsPy's classic_sta_lta,
 * recursive_sta_lta and trigger_onset (the reference's waveform check, volpick/data/utils.py:1064-1071), which
 * volpick_amd/trigger.py restates on the host.  With sq = x * x and tiny the smallest normal double:
 *
 *     VP_STALTA_RECURSIVE   csta = 1 / nsta, clta = 1 / nlta, sta = 0, lta = tiny, cft[0] = 0; for i = 1 .. n - 1:
 *                           sta = csta sq[i] + (1 - csta) sta, lta = clta sq[i] + (1 - clta) lta, cft[i] = sta / lta,
 *                           replaced by 0 where i < nlta.  Sample 0 never enters the sums.
 *     VP_STALTA_CLASSIC     STA[i], LTA[i]: the sum of sq over the nsta, nlta samples ending at i (samples ahead of the
 *                           series count as 0) divided by nsta, nlta; STA[i] = 0 for i < nlta - 1; LTA below tiny is
 *                           tiny; cft = STA / LTA.
 *
 * An all-zero series gives 0 everywhere (in the recursion also behind the sample where tiny (1 - clta)^i leaves the
 * doubles: 0 / lta stays 0); nlta > n gives all zeros.  in_dev: n_series series of n samples, series_stride samples from
 * one to the next (>= n), int32, float32 or float64 (in_kind).  out_dev: the same layout in float32 or float64 (out_kind:
 * VP_SAMPLES_FLOAT32 / FLOAT64); it must not overlap in_dev.  Arithmetic is float64 throughout, the only other rounding is
 * the store.  Every term is a square, so no sum here cancels: against the rule in extended precision the recursion is
 * within (6 (i + 1) + 10) 2^-53 of the value at sample i and the classic type within (nsta + nlta + 8) 2^-53 (the tests'
 * bars; float32 output adds 2^-24).
 *
 * Scheme: tiles of 8192 samples, pieces of 32.  Recursive: both states are linear in themselves, so they are carried
 * exactly as vp_sos_filter carries its state, with the host's table (1 - c)^(32 2^k), k = 0..15: per tile a scan of the
 * pieces' zero-state ends, one workgroup per series that scans the tiles' ends 256 at a time (lta's start value tiny is
 * its initial state), per tile the scan again and every piece run from its true start.  Classic: a window sum is never a
 * difference of running sums.  For each width w the series is cut into blocks of w samples; a window is the sum from its
 * first sample to the right edge of that sample's block plus the sum from the left edge of the next block to its last
 * sample.  Both are segmented scans (per tile, with the tiles' partial sums scanned by one workgroup per series, forward
 * and backward); a window of w samples takes at most w - 1 additions.  Order between tiles comes from the launch
 * boundaries alone; no atomics: the same call gives the same bits twice.
 *
 * Non-finite input: a NaN or an Inf is read as NaN.  Recursive: every sample >= max(first non-finite, nlta) is NaN, the head
 * stays 0 (sample 0, which never enters the sums, is not read: a non-finite value there changes nothing).  Classic: every sample at or after the first non-finite one is NaN, those below nlta - 1 included, as the rule's
 * whole-trace cumulative sum leaves them.  Samples ahead of the first non-finite one are right.  (ObsPy keeps an Inf as
 * Inf for the few samples until Inf - Inf or Inf / Inf turns it into NaN; here those are NaN at once.)
 *
 * VP_ERR_INVALID, out_dev untouched: a null pointer, an unknown in_kind, out_kind or type, n < 0, n_series < 1,
 * series_stride < n, nsta < 1, nsta > nlta, out_dev overlapping in_dev.  n == 0 does nothing.  VP_ERR_UNSUPPORTED, out_dev
 * untouched: nlta > 65536 (131 s at 500 Hz).  VP_ERR_NOMEM: the scratch cannot be allocated.  Runs on the device's null
 * stream and returns after the work is done, as vp_sos_filter does; calls on one device are serialised.
 *
 * The scratch (72 bytes per tile; 16 bytes per sample for the classic type) is kept per device, grow-only, between calls;
 * vp_sta_lta_release_scratch frees it and vp_trigger_onset's (bytes_freed may be NULL) -- the other release calls do not
 * touch it.  vp_sta_lta_bench: mean time in ms (HIP events on a stream of its own, three untimed repetitions first) of
 * `iters` repetitions of the whole call: bench only.
 *
 * vp_trigger_onset: trigger_onset(cft, thr_on, thr_off) without max_len for thr_off <= thr_on on n_series float32 rows in
 * device memory -- exactly the triggers of vp_pick, by the same scan kernel, without a vp_handle: a trigger opens at the
 * first sample > thr_on and closes at the last sample of the run of samples > thr_off; NaN compares false; peak / value are
 * the first maximum over [on, off].  Results as vp_classify_multi's: grouped by series (series_of, may be NULL), sorted by
 * onset, at most cap_per_series per series and cap in all; *n_found > cap means call again with more room (a series
 * that overflowed cap_per_series raises it above cap).  VP_ERR_INVALID: a null pointer, n < 0, n_series < 1,
 * series_stride < n, thr_off > thr_on (vp_pick_host has the general rule), a negative cap. */
enum { VP_STALTA_CLASSIC = 0, VP_STALTA_RECURSIVE = 1 };
int vp_sta_lta(int device_id, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n, int type,
               int64_t nsta, int64_t nlta, void* out_dev, int out_kind);
int vp_sta_lta_release_scratch(int device_id, size_t* bytes_freed);
int vp_sta_lta_bench(int device_id, const void* in_dev, int in_kind, int n_series, int64_t series_stride, int64_t n, int type,
                     int64_t nsta, int64_t nlta, void* out_dev, int out_kind, int iters, float* ms_total);
int vp_trigger_onset(int device_id, const float* cft_dev, int n_series, int64_t series_stride, int64_t n, float thr_on,
                     float thr_off, int64_t* on, int64_t* off, int64_t* peak, float* value, int32_t* series_of,
                     int cap_per_series, int cap, int* n_found);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU bring-up.  The reference is single-GPU; windows are independent given the
 * weights, so the one exchange is the start-up broadcast of the flat weight blob from the root rank: a single
 * ncclBroadcast over RCCL (xGMI inside a node), after which vp_create(..., VP_MEM_DEVICE, ...) builds the plan from the
 * received buffer.  One process per GPU.  RCCL is bound at run time (dlopen librccl.so.1).
 *
 * vp_rccl_unique_id: the root fills 128 bytes that every rank must receive out of band (a file, a socket,
 *   torch.distributed's store ...).  vp_rccl_comm_init: collective over the n_ranks processes, binds the communicator
 *   to device_id.  vp_bcast_weights: in place -- the root sends weights_dev, every other rank receives into it;
 *   returns when the data has arrived.  vp_rccl_comm_destroy releases the communicator.
 *
 * vp_rccl_available: 1 if RCCL could be bound in this process, 0 otherwise (vp_last_error says why).  A binder checks it
 *   on EVERY rank and agrees on the outcome (e.g. an all-reduce MIN over its own transport) before anyone enters the
 *   collective vp_rccl_comm_init: a rank that cannot take part must not leave the others waiting inside it. */
#define VP_RCCL_UNIQUE_ID_BYTES 128
int vp_rccl_available(void);
int vp_rccl_unique_id(void* id128);
int vp_rccl_comm_init(int device_id, int n_ranks, const void* id128, int rank, void** comm);
int vp_rccl_comm_info(void* comm, int* n_ranks, int* rank); /* ncclCommCount / ncclCommUserRank of the communicator */
int vp_rccl_comm_destroy(void* comm);
int vp_bcast_weights(void* rccl_comm, float* weights_dev, size_t n_floats, int root);
/* Absolute path of the shared object the RCCL entry points above were bound from (dladdr of ncclBroadcast), so that a
 * multi-GPU run can show that the process carries ONE RCCL: PyTorch-ROCm bundles a librccl with the same SONAME
 * (librccl.so.1), and dlopen by SONAME hands back the copy that is already mapped.  Writes a NUL-terminated string of at
 * most cap bytes; VP_ERR_UNSUPPORTED if RCCL could not be bound. */
int vp_rccl_library_path(char* buf, size_t cap);

const char* vp_last_error(void);
const char* vp_version(void);

/* ABI revision of this header.  It changes whenever a struct a caller fills (vp_config, vp_trigger_spec,
 * vp_mseed_record) changes size or layout, or an entry point changes its signature; added entry points do not bump it.
 * A binder compiled against this header checks vp_abi_version() == VP_ABI_VERSION and vp_config_size() ==
 * sizeof(vp_config) once, before vp_create reads its struct.  History: 1 = round 1 (vp_config with reserved[8]),
 * 2 = round 3 (plan_flags[8] + reserved[4]: the struct grew by 16 bytes), 3 = this header (layout of 2, the two
 * checks added). */
#define VP_ABI_VERSION 3
int vp_abi_version(void);
size_t vp_config_size(void);

#ifdef __cplusplus
}
#endif
#endif /* VOLPICK_HIP_H */
