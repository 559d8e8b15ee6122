/*
 * neuralaudio_amd.h -- additive C ABI of the MI355X-native library: the many-stream batch engine the
 * reference lacks, plus C access to the NeuralModel virtuals the legacy C API never exported.
 *
 * Plain pointers and sizes only (no C++/torch types).  Every function returning int returns 0 on success
 * and a negative value on failure; the failure text is available from NA_GetLastError() (thread-local).
 *
 * The batch is the data-parallel drop-in for "N hosts each calling NeuralModel::Process"
 * (NeuralAudio/NeuralModel.h:127): stream s of the batch is bit-for-bit what a single NeuralModel created
 * from the same file computes, so row s of `in`/`out` replaces the s-th host's Process(input, output, n).
 */
#ifndef NEURALAUDIO_AMD_H
#define NEURALAUDIO_AMD_H

#include "NeuralAudioCApi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct NA_Batch NA_Batch;

/* ---- library / device ------------------------------------------------------------------------- */
NA_EXTERN const char* NA_GetLastError(void);
NA_EXTERN int NA_GetDeviceCount(void);                 /* 0 when no HIP device / driver is present */
NA_EXTERN const char* NA_GetVersion(void);

/* ---- loader / model extras (NeuralModelLoader setters NeuralModel.h:155-221, virtuals :40-134) -- */
NA_EXTERN NeuralModel* NA_CreateModelFromFileUtf8(NeuralModelLoader* loader, const char* utf8Path, int doPrewarm);
NA_EXTERN NeuralModel* NA_CreateModelFromString(NeuralModelLoader* loader, const char* jsonText, const char* extension, int doPrewarm);
NA_EXTERN void NA_SetDevice(NeuralModelLoader* loader, int device);
/* activation arithmetic of the models created next: 0 = FastMath (default), 1 = StdMath -- the reference's build options
 * WAVENET_MATH / LSTM_MATH (NeuralAudio/CMakeLists.txt:82-96, Activation.h:12-118) as load-time knobs */
NA_EXTERN void NA_SetWaveNetMathMode(NeuralModelLoader* loader, int mathMode);
NA_EXTERN void NA_SetLSTMMathMode(NeuralModelLoader* loader, int mathMode);
/* ECompositeModelLoadMode (NeuralModel.h:27-31,166-174): 0 = LoadAll (default), 1 = OnDemand */
NA_EXTERN void NA_SetCompositeModelLoadMode(NeuralModelLoader* loader, int loadMode);
/* NeuralModel::IsQualityChangeRealtimeSafe (NeuralModel.h:54-59) */
NA_EXTERN int NA_IsQualityChangeRealtimeSafe(NeuralModel* model, float newQuality);
/* NeuralModel::Process with a status: 0 ok; on failure `output` is zero-filled (silence) and NA_GetLastError() says why.
 * The legacy Process() symbol forwards here and drops the status. */
NA_EXTERN int NA_ProcessChecked(NeuralModel* model, float* input, float* output, size_t numSamples);
NA_EXTERN void NA_SetDefaultQualityScaleFactor(NeuralModelLoader* loader, float quality);
NA_EXTERN void NA_SetExternalSampleRate(NeuralModelLoader* loader, int sampleRate);
NA_EXTERN int NA_HasQualityScaling(NeuralModel* model);
NA_EXTERN float NA_GetQualityScaleFactor(NeuralModel* model);
NA_EXTERN void NA_SetQualityScaleFactor(NeuralModel* model, float quality);
NA_EXTERN int NA_GetReceptiveFieldSize(NeuralModel* model);
NA_EXTERN int NA_Prewarm(NeuralModel* model);
/* copies the JSON text of a metadata field into buf (NUL-terminated, truncated); returns its full length */
NA_EXTERN int NA_GetMetadata(NeuralModel* model, const char* fieldName, char* buf, int bufSize);
NA_EXTERN int NA_GetModelVersion(NeuralModel* model, char* buf, int bufSize);

/* ---- batch engine -------------------------------------------------------------------------------- */
/* One batch == one GPU.  hipStream: NULL -> the batch creates its own non-blocking HIP stream;
 * otherwise the caller's hipStream_t is borrowed (e.g. torch.cuda.current_stream().cuda_stream). */
NA_EXTERN NA_Batch* NA_BatchCreate(int device, void* hipStream);
NA_EXTERN void NA_BatchDestroy(NA_Batch* batch);
/* Adds `count` streams running `model` (weights are shared on the device); returns the id (= row) of the
 * first one, ids are consecutive; negative on failure.  quality is used by SlimmableContainer models.
 * Ids retired by NA_BatchRemoveStreams are recycled first: the lowest retired id for count == 1, a run of `count` consecutive retired
 * ids when there is one; otherwise new rows are appended.  The device layout of a model's streams (e.g. narrow WaveNet models run
 * several streams per kernel-level stream) does not depend on how the streams arrived: 4096 single adds == one add of 4096. */
NA_EXTERN int NA_BatchAddStreams(NA_Batch* batch, NeuralModel* model, float quality, int count, int doPrewarm);
/* Stream lifetime = the reference's model lifetime (NeuralAudioCApi.cpp:38-42 DeleteModel): frees the device state of streams
 * [first, first + count) for recycling and retires their ids.  Rows keep their place in the [streams][n] arrays -- input ignored, host
 * output zero -- except trailing retired rows, which leave the arrays (check NA_BatchNumStreams afterwards).  Waits for the batch's
 * stream; call it between buffers, not from the audio callback.  Fails (negative) on ids that are out of range or already removed. */
NA_EXTERN int NA_BatchRemoveStreams(NA_Batch* batch, int first, int count);
/* ---- the stream pool: join and leave for a batch that never stops ----
 * NA_BatchReserveStreams is the set-up side (NOT real-time safe, like NA_BatchAddStreams): it creates `count` PARKED streams of `model`
 * and returns the first id (ids consecutive, retired ids recycled first, negative on failure).  Everything such a stream will ever need
 * on the device is created here -- rows, state slots of every submodel, index-list capacity, resampling histories, the half-batch
 * chains' streams, the staging of the re-arm -- and every parked stream is ARMED: its state is what NA_BatchAddStreams(count = 1,
 * doPrewarm) leaves behind, for every submodel of a slimmable model whatever the loader's composite load mode.  Stream packing of narrow
 * WaveNets is decided from `count` as NA_BatchAddStreams decides it, when this call creates the model group.
 * A parked stream keeps its row of the [streams][n] arrays like a retired one -- input ignored, host output zero, device output row left
 * alone; NA_BatchNumStreams does not change on activate / park -- and is not live: NA_BatchIsLive 0, not in NA_BatchNumLiveStreams;
 * NA_BatchSetQuality, NA_BatchPrewarm(stream), NA_BatchSaveStreams / LoadStreams fail on it ("... is parked"), NA_BatchPrewarm(-1) skips
 * it, NA_BatchRemoveStreams frees it like any stream (not real-time safe).
 * NA_BatchActivateStream (parked -> live, `quality` picks the submodel; fails on an id that is not parked) and NA_BatchParkStream (live
 * -> parked; fails on a stream that did not come from the pool) are REAL-TIME SAFE: host bookkeeping only.  The processing call that
 * follows enqueues the device work on the batch stream in front of the model launches -- the index-list upload, one re-arm launch per
 * model group, for a resampling batch the zeroing of the row's filter histories -- with no device or pinned allocation or free, no
 * stream or event creation and no host-side wait.  Three exceptions, all shared with NA_BatchSetQuality: a batch running its half-batch
 * chains or the resident launch drains them first (bounded by the wait limit); a batch of several launch units per buffer
 * re-captures its hipGraph; and a batch that runs more than eight different models of one kernel family (their launch takes its
 * group table from device memory) uploads that table again: a device free, an allocation and a blocking copy -- keep such a batch's
 * joins and leaves on the set-up side.  From its first sample an activated stream computes what a stream freshly added with
 * NA_BatchAddStreams(model, quality, 1, doPrewarm) computes, after every park -> activate cycle: a parked stream carries nothing over.
 * Streams that did not join or leave never notice.  A broken batch refuses all three calls. */
NA_EXTERN int NA_BatchReserveStreams(NA_Batch* batch, NeuralModel* model, int count, int doPrewarm);
NA_EXTERN int NA_BatchActivateStream(NA_Batch* batch, int stream, float quality);
NA_EXTERN int NA_BatchParkStream(NA_Batch* batch, int stream);
NA_EXTERN int NA_BatchIsParked(NA_Batch* batch, int stream);
NA_EXTERN int NA_BatchFindParked(NA_Batch* batch, NeuralModel* model); /* the lowest parked id of that model, -1: none */
NA_EXTERN int NA_BatchNumParked(NA_Batch* batch);
/* ---- the output stage: ramped stream gains and the click-free model switch ----
 * The output rows of NA_BatchProcessDevice and of the host-buffer paths never pass through host code that could scale or cross-fade
 * them; this is the place for it: a per-stream stage on the device, ONE launch per buffer behind the model launches, over the streams
 * that need it only.  A batch that enabled it and uses none of it launches exactly what it launched before.
 * NA_BatchEnableOutputStage is the set-up side (allocates; idempotent): it creates the stage's device + pinned tables for the batch's
 * current capacity; later NA_BatchAddStreams / NA_BatchReserveStreams grow them on the set-up side.  Every call below fails ("output
 * stage not enabled") before it.
 * Arithmetic -- all of it f32; positions count the samples the caller sees (in a resampling batch: external samples):
 *   Gain ramp.  A set call at the moment the stream's gain is g_a, with target g_b and length R, gives the k-th sample after the call
 *     (k = 0, 1, ...) the gain g_a + (g_b - g_a) * ((min(k, R-1) + 1) / R).  R = 0 means g_b from k = 0.  A set call during a ramp starts
 *     from the value the ramp has reached (g_a = the gain of the last sample produced): the gain never jumps.  `gain` must be finite
 *     and >= 0.  R and fadeSamples lie in [0, 1 << 20]: k + 1 is then exact in f32 and the ratio is one rounding.
 *   Fade.  For the k-th sample after NA_BatchHandover, w = (min(k, N-1) + 1) / N, and row `to` becomes
 *     (1 - w) * (g_from * y_from) + w * (g_to * y_to): y_* are the models' outputs, g_* the two streams' own (possibly ramping) gains.
 *     N = 0 means w = 1 at once: activate + park with nothing in between.  Row `from` keeps carrying g_from * y_from until it is
 *     parked.  The cross-fade is equal-gain, not equal-power: the two signals are two amps on the same input (correlated), so equal
 *     power would bump by 3 dB in the middle.
 *   Position.  w and the ramp value are computed from the absolute position, never accumulated sample to sample: the samples out do not
 *     depend on how the signal was cut into calls.
 * Host contract: from the call after NA_BatchHandover feed both rows the same input and listen to row `to`.  Nothing happens to the
 * session at the end of the fade except that `from` turns silent and returns to the pool, re-armed, as NA_BatchParkStream leaves it:
 * it is parked by the first processing call after the one that held the fade's last sample.  The incoming stream starts from its armed
 * (silence-prewarmed) state, as every joiner does; no input history is kept to warm it on the session's real past.
 * Rules (each fails with a message that names it, NA_GetLastError): `from` must be live and from the pool (NA_BatchParkStream refuses
 * others, and the hand-over ends in a park); `to` must be parked; neither may be part of a running fade, nor `from` a
 * stream whose fade has produced its last sample (the next processing call parks it); from != to; a broken batch refuses all the calls.  NA_BatchParkStream (or NA_BatchRemoveStreams, not real-time safe) on either stream of a running fade ends the
 * fade at the next buffer and the other stream carries on alone at its own gain: parking `to` cancels the fade, parking `from`
 * completes it at once.  Parking resets the stream's gain to 1: a parked stream carries nothing over.  Gains are not part of a
 * NA_BatchSaveStreams blob; NA_BatchLoadStreams leaves the destination's gain alone.
 * NA_BatchSetStreamGain and NA_BatchHandover are REAL-TIME SAFE: host arithmetic.  While an entry exists -- a stream with a gain != 1
 * or a running ramp, or a fade -- every processing call runs its launches in order on one stream (as a resampling batch does: no
 * half-batch chains, no resident launch; entering that path drains them under the wait limit, like a quality switch), enqueues one
 * table upload from a ring of pinned tables and the stage's launch, and host buffers go through the library's device staging block (a
 * registered block too; its first buffer of a new size allocates that block, as NA_BatchProcess on plain memory does).  No device or
 * pinned allocation besides, no stream or event creation, no unbounded wait; the activate and the later park follow the rules of
 * NA_BatchActivateStream / NA_BatchParkStream, exceptions included.  An entry retires when its ramp is finished at gain 1 and its
 * fade is over; with the last one the free-running modes come back. */
NA_EXTERN int NA_BatchEnableOutputStage(NA_Batch* batch);
NA_EXTERN int NA_BatchSetStreamGain(NA_Batch* batch, int stream, float gain, int rampSamples);
NA_EXTERN float NA_BatchGetStreamGain(NA_Batch* batch, int stream); /* the target; 1 for a stream that never had one; < 0: bad id */
NA_EXTERN int NA_BatchHandover(NA_Batch* batch, int from, int to, float quality, int fadeSamples);
NA_EXTERN int NA_BatchHandoverRemaining(NA_Batch* batch, int stream); /* samples left of the fade `stream` is part of (either side); 0: none; < 0: stage not enabled / bad id */
/* ---- the cabinet stage: per-stream impulse-response convolution ----
 * Almost every capture this library runs is an amp without its cabinet; a session becomes listenable once the model output has been
 * convolved with a cabinet impulse response (IR).  A host of the reference does that itself, with the samples in its hands; here the
 * rows stay on the device, so this is the place for it: a second per-stream stage behind the model launches (behind the down kernel of
 * a resampling batch) and in front of the output stage.  For every stream that has an IR the row's samples are replaced by their
 * convolution with that IR.  A batch that enabled the stage and assigned no IR launches exactly what it launched before.
 * Set-up side (not real-time safe: they allocate and may wait for what is in flight):
 *   NA_BatchEnableCabinetStage(maxTaps in [1, 8192]) allocates one history ring per row of the batch's capacity -- ringSamples floats,
 *     a power of two >= maxTaps - 1 + pieceSamples; pieceSamples is the longest run the stage processes at once, longer calls run in
 *     pieces -- and the stage's tables; later NA_BatchAddStreams / NA_BatchReserveStreams grow both.  Idempotent for an equal or
 *     smaller maxTaps; a larger maxTaps is refused while any stream has an IR.  Every call below fails ("cabinet stage not enabled")
 *     before it.  NA_BatchGetCabinetInfo reports the sizes in effect and the device memory the stage holds.
 *   NA_BatchLoadIR copies numTaps in [1, maxTaps] finite taps to the device and returns an IR id >= 0 (-1: failure); many streams may
 *     share one IR; ids of unloaded IRs are recycled.  Taps are given at the rate of the rows the caller sees (in a resampling batch:
 *     the external rate); the library does not resample IRs and reads no files.  NA_BatchUnloadIR fails while a stream uses the IR or
 *     fades from it.
 * Arithmetic -- all of it f32; positions count the samples the caller sees:
 *   y is the stream's row as the call would have produced it without this stage.  T0 is the position of the first sample after the
 *     set call that gave a dry stream an IR: y[t] = 0 for t < T0 (the history starts empty).
 *   For an IR h of K taps: c_h[t] = sum over k in [0, K) of h[k] * y[t - k].  The dry path is the one-tap IR {1}: c_dry[t] = y[t],
 *     bit for bit as a value.
 *   Fade.  NA_BatchSetStreamIR from A to B with length N gives the k-th sample after the call (1 - w) * c_A[t] + w * c_B[t], with
 *     w = (min(k, N-1) + 1) / N.  N = 0 means B from k = 0.  fadeSamples lies in [0, 1 << 20].  A switch between two IRs reads the same
 *     history, so it is exact: after the fade the row is what it would be had the stream had B since T0.  A switch from dry starts the
 *     history at T0; a stream that has faded to dry drops it.
 *   Summation order.  Products and sums are f32 FMAs; the order in which one output's K products are summed is a function of the tap
 *     index k and of K only (csrc/cabinet_stage.h): a sample's value does not depend on how the signal is cut into calls, on the
 *     sample's index in a call, on row alignment or stride, on how many entries the launch has, or on maxTaps.  Any order is within
 *     (K + 4) * 2^-24 * sum |h[k]| |y[t - k]| of the exact sum; integer taps and samples whose partial sums stay below 2^24 are exact.
 *   With the output stage.  Its y_from / y_to are this stage's outputs: every row is convolved with its own IR first, then scaled and
 *     cross-faded.  A preset change that keeps its cabinet: NA_BatchHandover(from, to, ...), then NA_BatchSetStreamIR(to, ir, 0).
 * Rules (each fails with a message that names it, NA_GetLastError): the stage must be enabled; the stream must be live (a parked one
 * fails with "... is parked"); the IR id must be loaded (or -1: dry); a set call while an IR fade of that stream is running is refused;
 * a broken batch refuses everything.  NA_BatchParkStream / NA_BatchRemoveStreams, and the park that ends a hand-over, make the stream
 * dry at once and drop its history: a parked stream carries nothing over, and an activated stream is dry.  IR assignment and history
 * are not part of a NA_BatchSaveStreams blob; NA_BatchLoadStreams leaves them alone.
 * NA_BatchSetStreamIR, NA_BatchGetStreamIR and NA_BatchStreamIRFadeRemaining are REAL-TIME SAFE: host arithmetic on tables that exist.
 * While an entry exists -- a stream with an IR, or a fade towards dry -- a processing call behaves as it does with output-stage
 * entries: its launches run in order on one stream (no half-batch chains, no resident launch), host buffers go through the library's
 * device staging block, and it enqueues one table upload from a ring of pinned tables plus two launches (append to the rings,
 * convolve) per piece of the call, over the streams with an entry only: no device or pinned allocation, no stream or event creation,
 * no unbounded wait.  The cost follows each IR's own length, not maxTaps.  When the last entry retires -- its fade to dry has
 * finished -- the free-running modes come back.
 * Not provided: the stage on NA_Multi* batches and on the one-stream NeuralModel; IR file reading; IR rate conversion; stereo IRs. */
typedef struct NA_CabinetInfo { int maxTaps, ringSamples, pieceSamples, numIRs; long long deviceBytes; } NA_CabinetInfo;
NA_EXTERN int NA_BatchEnableCabinetStage(NA_Batch* batch, int maxTaps);
NA_EXTERN int NA_BatchGetCabinetInfo(NA_Batch* batch, NA_CabinetInfo* info);
NA_EXTERN int NA_BatchLoadIR(NA_Batch* batch, const float* taps, int numTaps); /* an IR id >= 0; -1: failure */
NA_EXTERN int NA_BatchUnloadIR(NA_Batch* batch, int ir);
NA_EXTERN int NA_BatchSetStreamIR(NA_Batch* batch, int stream, int ir, int fadeSamples); /* ir = -1: none (dry) */
NA_EXTERN int NA_BatchGetStreamIR(NA_Batch* batch, int stream); /* the target: id, -1 dry, <= -2 bad id / not enabled */
NA_EXTERN int NA_BatchStreamIRFadeRemaining(NA_Batch* batch, int stream); /* samples left of the stream's IR fade; 0: none; < 0: stage not enabled / bad id */
/* ---- the reverb stage: per-stream convolution with a long impulse response ----
 * What a player hears behind a real rig is a room.  A room-mic cabinet IR is 0.3 - 1 s, a reverb IR 1 - 3 s; the cabinet stage is direct
 * form, ends at 8192 taps and costs what its taps cost.  This stage is uniformly partitioned FFT convolution: partitions of P = 128
 * samples, 256-point transforms, a per-row delay line of input spectra; the first 128 taps run direct form, so the stage has no
 * latency and a one-sample call works.  An eighth per-stream stage, off unless enabled, BEHIND the cabinet stage and IN FRONT OF the
 * output stage: a session's chain is model -> gate -> EQ -> cabinet -> reverb -> output gain -> mix (the delay stage, where enabled, sits between cabinet and reverb).  For every stream that has a reverb
 * the row's samples x are replaced by dry * x + wet * (x convolved with the IR).  A batch that enabled the stage and set no reverb
 * launches exactly what it launched before.  In a resampling batch the stage acts on the external-rate rows, as the cabinet does.
 * Set-up side (not real-time safe: they allocate and may wait for what is in flight):
 *   NA_BatchEnableReverbStage(maxTaps in [1, 131072]) allocates per row of the batch's capacity a ring of raw samples, a ring of
 *     `slots` input spectra of 2 KiB each (slots = ceil(maxTaps / 128) - 1 + the blocks a piece can touch; pieceSamples is the longest
 *     run the stage processes at once, longer calls run in pieces) and the tails of the blocks in work, and the stage's tables; later
 *     NA_BatchAddStreams / NA_BatchReserveStreams grow them.  Idempotent for an equal or smaller maxTaps; a larger maxTaps is refused
 *     while any stream has a reverb.  Every call below fails ("reverb stage not enabled") before it.  NA_BatchGetReverbInfo reports the
 *     sizes in effect and the device memory the stage holds.
 *   NA_BatchLoadReverbIR takes numTaps in [1, maxTaps] finite taps and returns an IR id >= 0 (-1: failure).  Taps [0, 128) go to the
 *     device as they are, the partitions behind them as spectra, computed on the device by the stage's own transform; the call waits
 *     for them under the wait limit.  Many streams may share one IR; ids of unloaded IRs are recycled.  Taps are given at the rate of
 *     the rows the caller sees.  NA_BatchUnloadReverbIR fails while a stream uses the IR or fades from it.
 * Arithmetic.  EVERY operation below is one f32 operation, rounded to nearest even, never contracted into an FMA, in the stated order;
 * f32 subnormals are kept, as operands and as results (nothing is flushed to zero).  Positions t count from T0, the first sample after
 * the set call that took the stream from no reverb: x[t] = 0 for t < 0 (the history starts empty; nothing is cleared on the device).
 * Block m is the samples [128 m, 128 m + 128).
 *   Twiddles.  W[q] = (cos(2 pi q / 256), -sin(2 pi q / 256)) for q in [0, 128), computed once on the host in double and rounded to f32.
 *   Complex product.  (a + bi)(c + di) = (a c - b d) + (a d + b c) i: four multiplies, one subtract, one add.
 *   Transform F of 256 complex values v: the FULL radix-2 decimation-in-time form -- all 256 complex bins are carried, also for real
 *     input (no real-input packing).  u[i] = v[i's 8 bits reversed]; for s = 1 .. 8, half = 2^(s-1), for every i in [0, 128):
 *     j = i mod half, top = 2 (i - j) + j, bot = top + half, p = W[j * 128 / half] * u[bot], u[bot] = u[top] - p, u[top] = u[top] + p.
 *     The product is taken also where W = (1, 0).  The inverse F' uses (Re W, -Im W) and no scale.
 *   Head.  head[t] = sum over k in [0, min(K, 128)) with k <= t of h[k] * x[t - k]: in rising k from +0, a multiply and then an add.
 *   Input spectra.  X_m = F([x block m-1, x block m]), imaginary parts +0, computed in the call that holds block m's last sample.
 *     They do not depend on the IR: a switch of IR continues on the history the old one saw.
 *   IR spectra.  H_j = F([h[128 j], ..., h[128 j + 127], 128 zeros]) for j = 1 .. J - 1, J = ceil(K / 128); taps past K are +0.
 *   Tail of block b.  A_b = sum over j in [1, min(J - 1, b)] of H_j * X_{b-j}: in rising j from (+0, +0), a complex product and then
 *     two adds -- an order that is a function of j alone.  tail[128 b + i] = Re(F'(A_b))[128 + i] * 2^-8 (the scale is exact).  It needs
 *     only blocks that are complete when block b begins; it is computed in the first call that needs it and kept for the rest of the block.
 *   Output.  c = head + tail;  y = (dry * x) + (wet * c).
 *   Fade.  NA_BatchSetStreamReverb with length N > 0 cross-fades between the whole outputs y_A, y_B of the old and the new setting
 *     (IR, wet, dry; "no reverb" has the output x itself): the k-th sample after the call is y_B where w = 1 and
 *     ((1 - w) * y_A) + (w * y_B) otherwise, w = (min(k, N-1) + 1) / N.  N = 0 means the new setting from k = 0, on the kept history.  A
 *     change of wet / dry on the same IR is such a fade.  fadeSamples lies in [0, 1 << 20].
 *   Consequence.  A sample's bits do not depend on how the signal is cut into calls, on the sample's index in a call, on row
 *     alignment or stride, on the other entries of the launch, or on maxTaps.  A restatement in f32 that follows the lines above
 *     operation for operation (tests/reverb_cases.py) is bit-exact.  Against the exact convolution the relative RMS error is about
 *     2e-7 for IRs of a few thousand taps.
 * Rules (each fails with a message that names it, NA_GetLastError): the stage must be enabled; the stream must be live (a parked one
 * fails with "... is parked"); the IR id must be loaded (or -1: no reverb); wet and dry must be finite; a set call while a reverb fade of
 * that stream is running is refused; a broken batch refuses everything.  NA_BatchParkStream / NA_BatchRemoveStreams, and the park that
 * ends a hand-over, take the reverb away at once and drop the history.  The stage's state is not part of a NA_BatchSaveStreams blob.
 * NA_BatchSetStreamReverb, NA_BatchGetStreamReverb and NA_BatchStreamReverbFadeRemaining are REAL-TIME SAFE: host arithmetic on tables
 * that exist.  While an entry exists -- a stream with a reverb, or a fade towards none -- a processing call runs its launches in order
 * on one stream, as with cabinet entries, and enqueues one table upload from a ring of pinned tables plus, per piece of the call and
 * over the streams with an entry only, the append and apply launches and -- where the piece completes a block / needs a tail -- the
 * spectrum and tail launches: no device or pinned allocation, no stream or event creation, no unbounded wait.  The tail's cost
 * follows each IR's own length, not maxTaps.
 * Not provided: non-uniform partitions; stereo IRs; the stage on NA_Multi* batches and on the one-stream NeuralModel; snapshots of the
 * stage's state; IR file reading or rate conversion. */
typedef struct NA_ReverbInfo { int maxTaps, partitionSamples, slots, pieceSamples, numIRs; long long deviceBytes; } NA_ReverbInfo;
NA_EXTERN int NA_BatchEnableReverbStage(NA_Batch* batch, int maxTaps);
NA_EXTERN int NA_BatchGetReverbInfo(NA_Batch* batch, NA_ReverbInfo* info);
NA_EXTERN int NA_BatchLoadReverbIR(NA_Batch* batch, const float* taps, int numTaps); /* an IR id >= 0; -1: failure */
NA_EXTERN int NA_BatchUnloadReverbIR(NA_Batch* batch, int ir);
NA_EXTERN int NA_BatchSetStreamReverb(NA_Batch* batch, int stream, int ir, float wet, float dry, int fadeSamples); /* ir = -1: no reverb */
NA_EXTERN int NA_BatchGetStreamReverb(NA_Batch* batch, int stream, float* wet, float* dry); /* the target: id (wet, dry filled; either may be NULL), -1 none, <= -2 bad id / not enabled */
NA_EXTERN int NA_BatchStreamReverbFadeRemaining(NA_Batch* batch, int stream); /* samples left of the stream's reverb fade; 0: none; < 0: stage not enabled / bad id */
/* ---- the delay stage: a per-stream echo, a feedback delay line ----
 * The block every guitar rig has between cabinet and room is a delay: echo, slap-back, dotted-eighth repeats.  A host of the reference
 * runs a delay on the buffer it holds.  Here the rows stay on the device, and an echo added by the host would come BEHIND the reverb:
 * the wrong order.  A ninth per-stream stage, off unless enabled, BEHIND the cabinet stage and IN FRONT OF the reverb stage: a session's
 * chain is model -> gate -> EQ -> cabinet -> delay -> reverb -> output gain -> mix.  (The compressor and modulation stages below sit between cabinet and delay.)  The line feeds back through a one-pole low-pass and
 * a one-pole high-pass, so the repeats darken and thin out as a tape echo's do.  In a resampling batch the stage acts on the
 * external-rate rows, as the cabinet does.  A batch that enabled the stage and set no delay launches exactly what it launched before.
 * Rows without an entry are never touched.
 * Set-up side (not real-time safe: it allocates and may wait for what is in flight):
 *   NA_BatchEnableDelayStage(maxDelaySamples in [1, 1 << 18]) allocates, per row of the batch's capacity, one ring of ringSamples floats
 *     and a small filter state, plus the stage's tables.  ringSamples is a power of two >= maxDelaySamples + pieceSamples;
 *     pieceSamples = 2048 is the longest run the stage processes at once, longer calls run in pieces.  Later NA_BatchAddStreams /
 *     NA_BatchReserveStreams grow the rings and tables.  Idempotent for an equal or smaller maximum; a larger one is refused while any
 *     stream has a delay.  Every other call fails with "delay stage not enabled (NA_BatchEnableDelayStage)" before it.
 *     NA_BatchGetDelayInfo reports the sizes in effect and the device memory the stage holds (deviceBytes: 512 MB for 1024 rows at a
 *     maximum of 2 s at 48 kHz, ringSamples = 131072).
 * Arithmetic.  Every floating-point operation is one separately rounded f32 operation, fl(.), rounded to nearest even, with no FMA
 * contraction.  f32 subnormals are kept as operands and as results.  Positions t = 0, 1, ... count the samples the caller sees since
 * T0, the first sample after the set call that took the stream from no delay.  The line starts empty: w[t] = 0 for t < 0, and nothing
 * is cleared on the device.  k is the count of samples since the last set call, an integer advanced by whole calls.
 * Constants of a setting: D = delaySamples in [1, maxDelaySamples]; fb = feedback, |fb| <= 0.99; aL = lowpassCoeff in (0, 1];
 * aH = highpassCoeff in [0, 1); wet, dry finite, |.| <= 1e6.  State per stream: the ring w, f32 l and q (both 0 at T0).
 * Per sample, in order, x the row's sample and y what replaces it:
 *   x' = isnan(x) ? 0 : clamp(x, +-1e18f)
 *   d  = w[t - D]                                       (+0 where t - D < 0)
 *   l  = (aL == 1) ? d : fl(l + fl(aL * fl(d - l)))     (aL == 1: l takes d, bit for bit)
 *   if aH == 0: h = l, q left alone;  else: q = fl(q + fl(aH * fl(l - q))), h = fl(l - q)
 *   w[t] = clamp(fl(x' + fl(fb * h)), +-1e30f)
 *   y  = (wet == 0) ? fl(dry * x') : fl(fl(dry * x') + fl(wet * h))
 * The clamps are exact min / max.  With the limits above every value stays finite whatever the input.
 * Set calls and fades.  A set call moves the stream from setting A to setting B over N = fadeSamples in [0, 1 << 20].  The weight is
 * the one the cabinet, EQ and reverb use: wk = 1 for k >= N - 1 and (float)(k + 1) / (float)N otherwise.  There is one ring and one
 * filter state throughout.
 *   The filter coefficients are B's from k = 0, on the kept l and q.
 *   fb, wet and dry each ramp: the value of a sample is B's where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk)); the step above runs
 *     on the ramped values (its test wet == 0 too).
 *   If D_A != D_B the read head cross-fades: d is w[t - D_B] where wk == 1, else
 *     fl(fl(fl(1 - wk) * w[t - D_A]) + fl(wk * w[t - D_B])).  If D_A == D_B there is no blend.
 *   "No delay" as A is B with wet = 0, dry = 1: a new delay fades in on an empty line.  As B (params == NULL) it is A with wet = 0,
 *     dry = 1: the echo fades out; the entry retires with the sample at which the fade ends -- later samples are not touched -- and
 *     the history is dropped.  With N = 0 it retires at once.
 *   A set call while a fade of that stream is running is refused.
 * Consequences.  A sample's bits do not depend on the cut into calls, on its index in a call, on alignment, on stride, on the other
 * entries or on maxDelaySamples.  With aL = 1, aH = 0 the line is pure arithmetic on taps: with fb = 0.5 and an impulse the echoes are
 * exact powers of two.  With wet = 0, dry = 1 the row is x' bit for bit.  A restatement in f32 that follows the lines above operation
 * for operation (tests/delay_cases.py) is bit-exact.
 * NA_DelayParamsFromMs is host arithmetic in double, rounded once: delaySamples = max(1, round(ms * rate / 1000)); lowpassCoeff = 1 when
 * highCutHz <= 0 or >= rate / 2, else 1 - exp(-2 pi highCutHz / rate); highpassCoeff = 0 when lowCutHz <= 0, else
 * 1 - exp(-2 pi lowCutHz / rate); wet = 10^(wetDb / 20) with -inf -> 0, dry likewise.  It refuses what the set call would refuse (a
 * delay beyond 1 << 18 samples included).  It needs no batch.
 * Rules (each fails with a message that names the field or the stream, NA_GetLastError): the stage must be enabled; the stream must be
 * live (a parked one fails with "... is parked"); every field must be within the limits above; a broken batch refuses everything.
 * NA_BatchParkStream / NA_BatchRemoveStreams, and the park that ends a hand-over, drop the delay and its history at once.  Delays are
 * not part of a NA_BatchSaveStreams blob.
 * NA_BatchSetStreamDelay, NA_BatchGetStreamDelay and NA_BatchStreamDelayFadeRemaining are REAL-TIME SAFE: host arithmetic on tables
 * that exist.  While an entry exists -- a stream with a delay, or a fade towards none -- a processing call behaves as it does with the
 * other stages' entries: it takes the ordered path, host buffers go through the staging block, and it enqueues one table upload from
 * the ring of pinned tables and one launch per piece over the entries only: no allocation, no stream or event creation, no unbounded
 * wait.  With the last entry the free-running modes come back.
 * Not provided: fractional or modulated delay times; ping-pong across rows; tempo helpers; the stage on NA_Multi* batches and on the
 * one-stream NeuralModel. */
typedef struct NA_DelayParams { int delaySamples; float feedback, lowpassCoeff, highpassCoeff, wet, dry; } NA_DelayParams;
typedef struct NA_DelayInfo   { int maxDelaySamples, ringSamples, pieceSamples, numDelays; long long deviceBytes; } NA_DelayInfo;
NA_EXTERN int NA_DelayParamsFromMs(int sampleRate, double delayMs, double feedback, double lowCutHz, double highCutHz, double wetDb, double dryDb, NA_DelayParams* out);
NA_EXTERN int NA_BatchEnableDelayStage(NA_Batch* batch, int maxDelaySamples);
NA_EXTERN int NA_BatchGetDelayInfo(NA_Batch* batch, NA_DelayInfo* info);
NA_EXTERN int NA_BatchSetStreamDelay(NA_Batch* batch, int stream, const NA_DelayParams* params, int fadeSamples); /* params = NULL: no delay */
NA_EXTERN int NA_BatchGetStreamDelay(NA_Batch* batch, int stream, NA_DelayParams* out); /* 1: *out filled (the target); 0: no delay (or a fade to none); < 0: stage not enabled / bad id */
NA_EXTERN int NA_BatchStreamDelayFadeRemaining(NA_Batch* batch, int stream); /* samples left of the stream's delay fade; 0: none; < 0: stage not enabled / bad id */
/* ---- the compressor stage: per-stream dynamics, a compressor or limiter ----
 * The one block of a guitar chain that was left to the host is dynamics: a compressor, or with an infinite ratio a limiter -- also the
 * block a server needs for its own safety, because two amps summed in a mix group, a makeup gain or a hot capture are not bounded by
 * anything else on the device.  A host of the reference compresses the buffer it holds.  Here the rows stay on the device, so it is a
 * tenth per-stream stage, off unless enabled, BEHIND the cabinet stage and IN FRONT OF the delay stage -- dynamics in front of the
 * time-based effects: a session's chain is model -> gate -> EQ -> cabinet -> compressor -> delay -> reverb -> output gain -> mix.  (The modulation stage below sits between compressor and delay.)  In
 * a resampling batch the stage acts on the external-rate rows, as the cabinet does.  A batch that enabled the stage and gave no
 * stream a compressor launches exactly what it launched before.  Rows without an entry are never touched.
 * Topology.  Feed-forward: a branching peak follower runs on the row's own samples, a static gain curve is read at the follower's
 * level, and the row is multiplied.  The gain computer has no transcendental on the device: a curve is a table of 513 gains on a level
 * axis that is the float's own bit pattern -- 16 knots per octave from 2^-24 to 2^8, interpolated linearly -- so compressor, limiter,
 * soft knee, makeup gain or any curve a caller designs himself are one mechanism, and the contract is exactly restatable.
 * Arithmetic.  Every operation is one separately rounded f32 operation, fl(.), round to nearest even.  There is no FMA contraction, and
 * subnormals are kept.
 *   Constants of an entry: aA = attackCoeff, aR = releaseCoeff in (0, 1].  Curve t[0..512], every value finite and in [0, 65536].
 *   Knot i sits at level 2^(-24 + (i >> 4)) * (1 + (i & 15) / 16).
 *   State per row: f32 e (starts at +0) and the last g.
 *   Per sample, x the row's sample:
 *     x' = (x is NaN) ? 0 : min(|x|, 255.0f)
 *     c  = (x' > e) ? aA : aR
 *     d  = fl(x' - e);  e = fl(e + fl(c * d))
 *     b  = bits(e);  q = b >> 19
 *     curve(t): q < 1648 ? t[0]
 *               : i = min(q - 1648, 511);  f = fl((float)(b & 0x7FFFF) * 2^-19);
 *                 fl(t[i] + fl(f * fl(t[i+1] - t[i])))
 *     g  = curve(tB)                                              where w == 1
 *     g  = fl(fl(fl(1 - w) * curve(tA)) + fl(w * curve(tB)))      else, w = OutStageWeightAt(N, k)
 *     y  = fl(x * g)
 *   w = OutStageWeightAt(N, k) is the fade weight of the other stages, (min(k, N - 1) + 1) / N for the k-th sample since the set call.
 *   e never leaves [0, 2^8), so i + 1 <= 512: x' lies in [0, 255] and c in (0, 1]; where x' > e, fl(c * d) <= d = fl(x' - e) because
 *   rounding is monotone, so the new e is at most fl(e + d) <= 255 + 2^-16 and at least e; where x' <= e, |fl(c * d)| <= |d| <= e, so
 *   the new e lies in [0, e], and an exact cancellation gives +0, never -0.  Hence bits(e) < bits(256.0f) and q <= 1648 + 511.
 *   A NaN or infinite sample goes through the multiplication as it is.  The follower sees 0 or 255.
 *   A row has two curve slots, as the EQ has two cascades.  tB is the curve it has or fades to.  tA is the one it fades from.  "No
 *   compressor" is the unity curve: g = 1, never read from memory.
 * Consequences: the bits do not depend on how the signal is cut into calls, on alignment, stride, the other streams or in-place use;
 * an all-ones curve passes the row bit for bit; with aA = aR = 1, samples from {0, +-0.5, +-2} and t[i] = 1 for i < 384, 0.25 for
 * i >= 384, y is x at |x| = 0.5 and exactly x / 4 at |x| = 2 (knot 384 is level 1.0, knot 368 is level 0.5).
 * NA_CompressorParamsFromDb is host arithmetic and needs no device.  Coefficients are 1 - exp(-1 / (ms * rate / 1000)) in double,
 *   rounded once (the gate's formula); ms == 0 gives 1.  Per knot, in double, with L = 20 log10(level_i), o = L - thresholdDb,
 *   s = 1 / ratio - 1 (ratio in [1, +inf], +inf gives s = -1) and W = kneeDb >= 0:
 *     G = 0 if 2o < -W;   G = s (o + W/2)^2 / (2W) if 2|o| <= W;   G = s o else;   t[i] = (float)10^((G + makeupDb) / 20).
 *   Every bad field is refused by name (sampleRate, thresholdDb, ratio, kneeDb, makeupDb, attackMs, releaseMs; a gain outside
 *   [0, 65536] names the knot).  Between knots the linear interpolation of a power-law stretch of slope s is off by at most
 *   |s (s - 1)| / 2048 relative (0.0085 dB for a limiter); a segment that straddles a corner is off by at most
 *   |s| * 20 log10(17 / 16) / 4 dB (0.13 dB for a limiter with a hard knee).
 * NA_BatchEnableCompressorStage is the set-up side (allocates; idempotent): two curve slots and a state per row (4232 bytes) and the
 *   stage's device + pinned tables, sized so that every row's entry and the curves of both its slots fit one table; later
 *   NA_BatchAddStreams / NA_BatchReserveStreams grow them.  Every call below fails before it, with
 *   "compressor stage not enabled (NA_BatchEnableCompressorStage)".  NA_BatchGetCompressorInfo reports curvePoints = 513, the number
 *   of entries and the device memory the stage holds.
 * NA_BatchSetStreamCompressor is REAL-TIME SAFE: host arithmetic on tables that exist.
 *   A set call on a stream without a compressor fades in from unity over fadeSamples with e = +0.
 *   On a stream with a compressor the new curve fades in over fadeSamples from the curve it has.  New aA / aR act from the next sample
 *     on the kept e.  Only curves fade.
 *   params == NULL fades to unity, and the entry retires when the fade ends (the follower goes on with the coefficients it has).  On
 *     a stream without a compressor it does nothing.
 *   fadeSamples == 0 switches at the next sample; fadeSamples must lie in [0, 1 << 20].
 *   A set call while a fade is running is refused with an error that gives the samples left ("a compressor fade of stream <s> is
 *     running (<k> samples left)").  The caller polls NA_BatchStreamCompressorFadeRemaining.
 *   Curves travel once, behind the table of the first call after the set call, from pinned memory sized at enable time.
 *   attackCoeff and releaseCoeff must lie in (0, 1]; every curve value must be finite and lie in [0, 65536].  Each failure names the
 *     field ("curve[<i>] must ...").
 * NA_BatchGetStreamCompressor returns 1 and fills *out with the target, 0 when the stream has no compressor or one that fades to none,
 *   < 0 on a bad id or when the stage is not enabled.  NA_BatchStreamCompressorGain returns the g of the last sample produced (1
 *   without a compressor or before its first sample, < 0 on a bad id); it reads the device state and synchronises the batch: a
 *   diagnostic like NA_BatchStreamGateGain, not for the audio callback.
 * Rules (each fails with a message that names it, NA_GetLastError): the stage must be enabled; the stream must be live (a parked one
 * fails with "... is parked"); a broken batch refuses everything.  NA_BatchParkStream / NA_BatchRemoveStreams, and the park that ends a
 * hand-over, drop the compressor at once: a parked stream carries nothing over, and an activated stream has none.  Compressors are not
 * part of a NA_BatchSaveStreams blob; NA_BatchLoadStreams leaves them alone.
 * While an entry exists -- a stream with a compressor, or a fade towards none -- a processing call behaves as it does with entries of
 * the other stages: its launches run in order on one stream (no half-batch chains, no resident launch), host buffers go through the
 * library's device staging block, and it enqueues one table upload from a ring of pinned tables plus ONE launch over the compressed
 * streams only, whatever n: no device or pinned allocation, no stream or event creation, no unbounded wait.  With the last entry the
 * free-running modes come back.
 * Not provided: the stage on NA_Multi* batches and on the one-stream NeuralModel; a gain-reduction tap in the meter stage; a side chain
 * on the dry input; stereo linking across a mix group; look-ahead. */
typedef struct NA_CompressorParams { float attackCoeff, releaseCoeff; float curve[513]; } NA_CompressorParams;
typedef struct NA_CompressorInfo { int curvePoints, numCompressors; long long deviceBytes; } NA_CompressorInfo;
NA_EXTERN int NA_CompressorParamsFromDb(int sampleRate, float thresholdDb, float ratio, float kneeDb, float makeupDb, float attackMs, float releaseMs, NA_CompressorParams* out);
NA_EXTERN int NA_BatchEnableCompressorStage(NA_Batch* batch);
NA_EXTERN int NA_BatchGetCompressorInfo(NA_Batch* batch, NA_CompressorInfo* info);
NA_EXTERN int NA_BatchSetStreamCompressor(NA_Batch* batch, int stream, const NA_CompressorParams* params, int fadeSamples); /* params = NULL: the compressor goes, click-free */
NA_EXTERN int NA_BatchGetStreamCompressor(NA_Batch* batch, int stream, NA_CompressorParams* out); /* 1: *out filled (the target); 0: none (or a fade to none); < 0: stage not enabled / bad id */
NA_EXTERN int NA_BatchStreamCompressorFadeRemaining(NA_Batch* batch, int stream); /* samples left of the stream's curve fade; 0: none; < 0: stage not enabled / bad id */
NA_EXTERN float NA_BatchStreamCompressorGain(NA_Batch* batch, int stream); /* the g of the last sample produced; 1: no compressor; < 0: bad id / not enabled */
/* ---- the modulation stage: per-stream chorus, flanger, vibrato and tremolo ----
 * A guitar rig has modulation between dynamics and echo, and the delay stage above reads its line at an integer delay that is constant
 * for a call.  A host that added a chorus itself would add it BEHIND reverb and mix, or give up the zero-copy path.  So it is an
 * eleventh per-stream stage, off unless enabled, BEHIND the compressor stage and IN FRONT OF the delay stage: a session's chain is
 * model -> gate -> EQ -> cabinet -> compressor -> modulation -> delay -> reverb -> output gain -> mix.  In a resampling batch the stage
 * acts on the external-rate rows, as the cabinet does.  A batch that enabled the stage and set nothing launches exactly what it launched
 * before.  Rows without an entry are never touched.
 * One mechanism: up to four voices read a short line w of the row's own samples at a fractional delay that an LFO sweeps between
 * baseSamples and baseSamples + depthSamples; the first voice may feed back into the line; the voices' sum is mixed with the dry sample;
 * the result may be scaled by the LFO.  A chorus is three voices a third of a cycle apart around 7 ms; a flanger one voice around 1 ms
 * with feedback; a vibrato one voice with dry = 0; a tremolo wet = 0 and tremoloDepth > 0.
 * Set-up side (not real-time safe: it allocates and may wait for what is in flight):
 *   NA_BatchEnableModStage(maxDelaySamples in [8, 4096]) allocates, per row of the batch's capacity, one ring of ringSamples floats, plus
 *     the stage's tables.  ringSamples is a power of two >= maxDelaySamples + pieceSamples; pieceSamples = 2048 is the longest run the
 *     stage processes at once, longer calls run in pieces: 16 KB or 32 KB a row, at most 32 MB for 1024 rows.  Later NA_BatchAddStreams /
 *     NA_BatchReserveStreams grow the rings and tables; the lines of streams that play are kept.  Idempotent for an equal or smaller
 *     maximum; a larger one is refused while any stream has a modulation.  Every other call fails with
 *     "modulation stage not enabled (NA_BatchEnableModStage)" before it.  NA_BatchGetModInfo reports the sizes in effect, the number of
 *     entries and the device memory the stage holds (deviceBytes).
 * Arithmetic.  Every floating-point operation is one separately rounded f32 operation, fl(.), rounded to nearest even, with no FMA
 * contraction.  f32 subnormals are kept as operands and as results.  Integers are exact.
 * Positions.  t counts the samples since T0, the first sample after the set call that took the stream from no modulation.  k counts the
 * samples since the last set call.  The line starts empty: w[t] = +0 for t < 0, decided by comparing positions, never by what the ring
 * holds; nothing is cleared on the device.
 * Limits of a setting: baseSamples >= 2; depthSamples >= 0; fl(baseSamples + depthSamples) <= maxDelaySamples - 2; numVoices in [1, 4];
 * |voiceGain| <= 4; |feedback| <= 0.95; wet and dry finite, |.| <= 1e6; tremoloDepth in [0, 1]; shape is NA_MOD_TRIANGLE or NA_MOD_SINE.
 * LFO, with no transcendental and no accumulation:
 *   u_v = phaseAtSet + (unsigned)(k * phaseInc) + voicePhase[v]                 (modulo 2^32: the low word of the 64-bit product)
 *   h   = (u_v & 0x80000000) ? ~u_v : u_v
 *   tri = fl((float)(h >> 7) * 2^-24)                                           (exact, in [0, 1))
 *   s_v = tri                                                                   for NA_MOD_TRIANGLE
 *   s_v = min(fl(fl(tri * tri) * fl(3 - fl(2 * tri))), 1)                       for NA_MOD_SINE: the smoothstep of the triangle
 *   phaseAtSet is 0 at T0.  Every set call advances it by the old (unsigned)(k * phaseInc): a new rate acts at once on a continuous phase.
 *   Both shapes stay in [0, 1] for every one of the 2^24 values of tri.  The "sine" lies within about 0.01 of the raised cosine
 *   (1 - cos(pi tri)) / 2 (measured maximum 0.010009, at tri = 0.7215 and its mirror; tests/test_mod_cpu.py).
 * Per sample, in order, x the row's sample and y what replaces it; base, depth, fb, wet, dry, td = tremoloDepth and the gains g_v are
 * the (ramped) values of the sample:
 *   x'    = isnan(x) ? 0 : clamp(x, +-1e18f)
 *   per voice v < numVoices:
 *     D   = fl(base + fl(depth * s_v));  Di = (int)D;  fr = fl(D - (float)Di)
 *     a   = w[t - Di];  b = w[t - Di - 1]                                       (+0 in front of the line's start)
 *     tap_v = fl(a + fl(fr * fl(b - a)))
 *   m     = fl(g_0 * tap_0), then m = fl(m + fl(g_v * tap_v)) in voice order
 *   w[t]  = (fb == 0) ? x' : clamp(fl(x' + fl(fb * tap_0)), +-1e30f)
 *   y0    = (wet == 0) ? fl(dry * x') : fl(fl(dry * x') + fl(wet * m))
 *   y     = (td == 0) ? y0 : fl(y0 * fl(1 - fl(td * s_0)))
 * The clamps are exact min / max.  With the limits above every value stays finite whatever the input.
 * Set calls and fades.  A set call moves the stream from setting A to setting B over N = fadeSamples in [0, 1 << 20], with the weight
 * the other stages use: wk = 1 for k >= N - 1 and (float)(k + 1) / (float)N otherwise.
 *   base, depth, fb, wet, dry, td and the four voice gains each take B's value where wk == 1, else fl(g_A + fl(fl(g_B - g_A) * wk)).  The
 *     delay is fractional already, so a new delay time glides: there is no read-head cross-fade.
 *   A voice absent from a setting has gain 0 in it.
 *   numVoices, voicePhase and phaseInc are B's from k = 0.  A set call that changes voicePhase[v] of a voice whose gain in A is non-zero
 *     is refused by name ("voicePhase[<v>] of a sounding voice must not change").
 *   If the shapes differ, s_v = fl(fl(fl(1 - wk) * sA_v) + fl(wk * sB_v)) while wk != 1.
 *   "None" as A is B with wet = 0, dry = 1, td = 0, fb = 0: a new effect fades in on an empty line.
 *   "None" as B (params == NULL) is A with wet = 0, dry = 1, td = 0: the effect fades out; the entry retires with the sample at which the
 *     fade ends -- later samples of that call's row are not touched -- and the history is dropped.  With N = 0 it retires at once.
 *   A set call while a fade of that stream is running is refused with the samples left ("a modulation fade of stream <s> is running
 *     (<k> samples left)").  The caller polls NA_BatchStreamModFadeRemaining.
 * Consequences.  A sample's bits do not depend on the cut into calls, on alignment, on stride, on in-place use, on the other entries or
 * on maxDelaySamples.  With wet = 0, dry = 1, td = 0 the row is x' bit for bit.  With depth = 0, an integer base = D, one voice of gain 1,
 * wet = 1, dry = 0 and fb = 0.5 an impulse gives exact powers of two at the multiples of D, down through the subnormals.  With
 * base = D + 0.5 and fb = 0 an impulse gives exactly 0.5 at D and at D + 1.  With td = 1, wet = 0, dry = 1 and a constant input of 1,
 * y = fl(1 - s_0).  A restatement in f32 that follows the lines above operation for operation (tests/mod_cases.py) is bit-exact.
 * NA_ModParamsFromMs is host arithmetic in double, each value rounded once: baseSamples and depthSamples are ms * rate / 1000;
 * phaseInc = round(rateHz / rate * 2^32), rateHz in [0, rate / 2]; voicePhase[v] = floor(v * 2^32 / voices); voiceGain[v] = 1 / voices;
 * wet = 10^(wetDb / 20) with -inf -> 0, dry likewise.  It refuses what the set call would refuse (a reach beyond 4094 samples
 * included).  It needs no batch.
 * Rules (each fails with a message that names the field or the stream, NA_GetLastError): the stage must be enabled; the stream must be
 * live (a parked one fails with "... is parked"); every field must be within the limits above; a broken batch refuses everything.
 * NA_BatchParkStream / NA_BatchRemoveStreams, and the park that ends a hand-over, drop the modulation and its history at once.
 * Modulations are not part of a NA_BatchSaveStreams blob.
 * NA_BatchSetStreamMod, NA_BatchGetStreamMod and NA_BatchStreamModFadeRemaining are REAL-TIME SAFE: host arithmetic on tables that
 * exist.  While an entry exists -- a stream with a modulation, or a fade towards none -- a processing call behaves as it does with the
 * other stages' entries: it takes the ordered path, host buffers go through the staging block, and it enqueues one table upload from
 * the ring of pinned tables and one launch per piece over the entries only: no allocation, no stream or event creation, no unbounded
 * wait.  With the last entry the free-running modes come back.
 * Not provided: the stage on NA_Multi* batches and on the one-stream NeuralModel; more than four voices; through-zero flanging; a phaser
 * (all-pass stages); stereo spread across the rows of a mix group; tempo helpers. */
#define NA_MOD_TRIANGLE 0
#define NA_MOD_SINE     1
typedef struct NA_ModParams { float baseSamples, depthSamples; unsigned phaseInc; int shape, numVoices;
                              unsigned voicePhase[4]; float voiceGain[4]; float feedback, wet, dry, tremoloDepth; } NA_ModParams; /* 68 bytes */
typedef struct NA_ModInfo   { int maxDelaySamples, ringSamples, pieceSamples, numMods; long long deviceBytes; } NA_ModInfo;
NA_EXTERN int NA_ModParamsFromMs(int sampleRate, double baseMs, double depthMs, double rateHz, int shape, int voices,
                                 double feedback, double wetDb, double dryDb, double tremoloDepth, NA_ModParams* out);
NA_EXTERN int NA_BatchEnableModStage(NA_Batch* batch, int maxDelaySamples);     /* [8, 4096]; idempotent for equal or smaller; larger refused while entries exist */
NA_EXTERN int NA_BatchGetModInfo(NA_Batch* batch, NA_ModInfo* info);
NA_EXTERN int NA_BatchSetStreamMod(NA_Batch* batch, int stream, const NA_ModParams* params, int fadeSamples);  /* params = NULL: the effect goes, click-free */
NA_EXTERN int NA_BatchGetStreamMod(NA_Batch* batch, int stream, NA_ModParams* out); /* 1: *out filled (the target); 0: none (or a fade to none); < 0: stage not enabled / bad id */
NA_EXTERN int NA_BatchStreamModFadeRemaining(NA_Batch* batch, int stream); /* samples left of the stream's modulation fade; 0: none; < 0: stage not enabled / bad id */
/* ---- the gate stage: a per-stream noise gate ----
 * High-gain captures turn pickup hum into a loud hiss between notes.  A host of the reference gates that itself: it listens to the dry
 * input and scales the amp's output, because it holds both buffers.  Here the rows stay on the device, and a gate needs both ends of a
 * processing call -- the input rows before the models run and the output rows after them -- so it is a stage of the library: a third
 * per-stream stage, off unless enabled.  A batch that enabled it and set no gate launches exactly what it launched before.
 * Order of a processing call: the gate DETECTOR in front of everything -- it reads the input rows as the caller passed them (in a
 * resampling batch: the external-rate rows; input and output rows may be the same memory) -- then the up kernel, the model launches
 * and the down kernel as before, then the gate APPLY, the cabinet stage and the output stage.  The gate scales the amp's output in
 * front of the cabinet, so the cabinet's tail rings out through a closing gate.  In a resampling batch the gain g[t] computed from
 * input sample t multiplies output sample t of the caller's row: the audio lags the gain by latencySamples (NA_BatchGetResampleInfo),
 * which acts as a small look-ahead; it is not compensated.
 * Arithmetic.  All floating-point operations are separately rounded f32 operations in this order, with no FMA contraction (fl(.) is
 * one rounding to f32, round to nearest even), so that a float32 restatement is bit-exact and the samples out do not depend on how
 * the signal is cut into calls.
 *   Constants of an entry: a = detectorCoeff in (0, 1]; Po = openPower >= Pc = closePower >= 0, thresholds as power; H = holdSamples;
 *     A = attackSamples, R = releaseSamples; floor = floorGain in [0, 1], the gain of the closed gate.
 *   Derived: span = fl(1 - floor), computed once on the host; U = 2^30; stepUp = ceil(U / A); stepDown = ceil(U / R).
 *   State per stream: f32 p, integer hold, bit open, unsigned u in [0, U].
 *   For each sample, in order, with x the input sample and y the row's sample after the models:
 *     x' = (x is NaN) ? 0 : min(|x|, 1e18f)
 *     s = fl(x' * x');  d = fl(s - p);  p = fl(p + fl(a * d))
 *     if      p >= Po:  open = 1, hold = H
 *     else if p <  Pc:  if hold > 0: hold -= 1  else: open = 0
 *     (between the thresholds nothing changes)
 *     u = open ? min(U, u + stepUp) : (u > stepDown ? u - stepDown : 0)
 *     g = (u == U) ? 1.0f : fl(floor + fl(span * fl((float)u * 2^-30)))
 *     y = fl(y * g)
 *   (float)u is round-to-nearest-even.  u is an integer on purpose: a gate that has been open for A samples is at exactly g = 1 and
 *   passes the row bit for bit, a closed gate with floor = 0 gives exact zeros, and the host can tell from sample counts alone when a
 *   ramp has ended.
 * NA_GateParamsFromDb is host arithmetic and needs no device: thresholds are dBFS of a sine's peak, so power = 10^(dB/10) / 2;
 *   floorGain = 10^(floorDb/20), a floorDb of -inf gives 0; detectorCoeff = 1 - exp(-1 / (ms * rate / 1000)), computed in double and
 *   rounded once; sample counts are max(1, round(ms * rate / 1000)), hold may be 0.  It refuses what the set call would refuse.
 * NA_BatchEnableGateStage is the set-up side (allocates; idempotent): a state per row, a gain block of gainSamples floats per row
 *   (a power of two >= 2048) and the stage's device + pinned tables; later NA_BatchAddStreams / NA_BatchReserveStreams grow them.  A
 *   processing call longer than gainSamples grows the gain block first: that growth is not real-time safe -- the rule for the first
 *   use of a longer buffer.  Every call below fails ("gate stage not enabled (NA_BatchEnableGateStage)") before it.
 *   NA_BatchGetGateInfo reports gainSamples, the number of entries and the device memory the stage holds.
 * NA_BatchSetStreamGate is REAL-TIME SAFE: host arithmetic on tables that exist.
 *   The stream has no gate: the gate starts at the next sample, from p = 0, open = 1, hold = H, u = U (startOpen != 0) or from p = 0,
 *     open = 0, hold = 0, u = 0 (startOpen == 0: for the `to` stream of a hand-over whose session is gated shut).
 *   The stream has a gate: the new constants apply from the next sample; the state is kept, with hold = min(hold, H); startOpen is
 *     ignored.
 *   params == NULL takes the gate away, click-free: the entry stays with `open` forced to 1 (the follower and the hold counter go on)
 *     and retires once attackSamples samples have been produced since the call; u == U by then, by construction.  A set call during
 *     that tail re-arms the gate on the kept state.  On a stream without a gate it does nothing.
 *   Every float must be finite; openPower >= closePower >= 0; floorGain in [0, 1]; detectorCoeff in (0, 1]; attackSamples and
 *     releaseSamples in [1, 1 << 20]; holdSamples in [0, 1 << 24].  Each failure names the field.
 * NA_BatchGetStreamGate returns 1 and fills *out with the constants in effect, 0 when the stream has no gate or one that is being taken
 *   away, < 0 on a bad id or when the stage is not enabled.  NA_BatchStreamGateGain returns the g of the last sample produced (1 for a
 *   stream without a gate, < 0 on a bad id); it reads the device state and synchronises the batch: a diagnostic like
 *   NA_BatchStreamRangeEvents, not for the audio path.
 * Rules (each fails with a message that names it, NA_GetLastError): the stage must be enabled; the stream must be live (a parked one
 * fails with "... is parked"); a broken batch refuses everything.  NA_BatchParkStream / NA_BatchRemoveStreams, and the park that ends a
 * hand-over, drop the gate at once: a parked stream carries nothing over, and an activated stream has none.  Gates are not part of a
 * NA_BatchSaveStreams blob; NA_BatchLoadStreams leaves them alone.
 * While an entry exists -- a stream with a gate, or one whose gate is being taken away -- a processing call behaves as it does with
 * entries of the other stages: its launches run in order on one stream (no half-batch chains, no resident launch), host buffers go
 * through the library's device staging block, and it enqueues one table upload from a ring of pinned tables plus two launches
 * (detector, apply) over the gated streams only, whatever n: no device or pinned allocation, no stream or event creation, no unbounded
 * wait.  With the last entry the free-running modes come back.
 * Not provided: the stage on NA_Multi* batches and on the one-stream NeuralModel; a side-chain input.  (Gain-reduction meters that are
 * safe to read from the audio thread are the GATE tap of the meter stage, below.) */
typedef struct NA_GateParams { float openPower, closePower, floorGain, detectorCoeff; int attackSamples, holdSamples, releaseSamples; } NA_GateParams;
typedef struct NA_GateInfo { int gainSamples, numGates; long long deviceBytes; } NA_GateInfo;
NA_EXTERN int NA_GateParamsFromDb(int sampleRate, float openDb, float closeDb, float floorDb, float detectorMs, float attackMs, float holdMs, float releaseMs, NA_GateParams* out);
NA_EXTERN int NA_BatchEnableGateStage(NA_Batch* batch);
NA_EXTERN int NA_BatchGetGateInfo(NA_Batch* batch, NA_GateInfo* info);
NA_EXTERN int NA_BatchSetStreamGate(NA_Batch* batch, int stream, const NA_GateParams* params, int startOpen); /* params = NULL: the gate goes, click-free */
NA_EXTERN int NA_BatchGetStreamGate(NA_Batch* batch, int stream, NA_GateParams* out); /* 1: filled; 0: no gate; < 0: bad id / not enabled */
NA_EXTERN float NA_BatchStreamGateGain(NA_Batch* batch, int stream); /* the g of the last sample produced; 1: no gate; < 0: bad id / not enabled */
/* ---- the EQ stage: a per-stream tone stack ----
 * Between the amp and the cabinet a session has its tone stack: bass, mid and treble shelves and peaks, usually with a high-pass and a
 * low-pass around them.  A host of the reference runs a few biquads on the buffer it holds.  Here the rows stay on the device between
 * the model launches and the cabinet stage, so the EQ is a stage of the library: a fourth per-stream stage, off unless enabled -- a
 * cascade of up to NA_EQ_MAX_SECTIONS biquad sections per stream, applied to the row the models produced BEHIND the gate's apply and IN
 * FRONT OF the cabinet stage.  A session's chain is model -> gate -> EQ -> cabinet -> reverb -> output gain -> mix (the delay stage, where enabled, sits between cabinet and reverb).  In a resampling batch the stage
 * acts on the external-rate rows, behind the down kernel, as the cabinet does: coefficients are designed at the rate the caller sees.
 * A batch that enabled the stage and gave no stream an EQ launches exactly what it launched before.
 * Arithmetic.  Every floating-point operation below is one separately rounded IEEE operation (fl(.): f64, fl32(.): f32, round to
 * nearest even) with no FMA contraction; f64 and f32 subnormals are kept.  A restatement in double is therefore bit-exact, and the
 * samples out do not depend on how the signal is cut into calls, on alignment, on stride, on the other streams or on the sample's
 * index in a call.
 *   Input: the sample is sanitised in f32, then widened exactly:
 *     x' = isnan(x) ? 0 : clamp(x, +-1e18f);  v0 = (double)x'
 *   Section i of a cascade keeps four doubles x1, x2, y1, y2 (direct form I).  Per sample, for sections 0 .. S-1 in order:
 *     acc = fl(b0*v); acc = fl(acc + fl(b1*x1)); acc = fl(acc + fl(b2*x2));
 *     acc = fl(acc - fl(a1*y1)); acc = fl(acc - fl(a2*y2));
 *     x2 = x1; x1 = v; y2 = y1; y1 = acc; v = acc
 *   Output: o = (float)v, rounded to nearest even once.  A cascade of 0 sections is the identity on x'.
 * NA_EqSectionFromDesign is host arithmetic and needs no device: the RBJ cookbook in double, Q form -- w0 = 2 pi f / Fs,
 *   alpha = sin(w0) / (2 Q), A = 10^(dB / 40), divided through by a0.  kind: 0 low-pass, 1 high-pass, 2 low shelf, 3 high shelf,
 *   4 peaking; gainDb matters for the shelves and the peak only.  It refuses a non-finite argument, freqHz outside (0, Fs / 2), q <= 0,
 *   an unknown kind, and anything the set call would refuse.
 * NA_BatchEnableEqStage is the set-up side (allocates; idempotent): two slots of coefficients and section states per row and the
 *   stage's device + pinned tables; later NA_BatchAddStreams / NA_BatchReserveStreams grow them.  Every call below fails ("eq stage not
 *   enabled (NA_BatchEnableEqStage)") before it.  NA_BatchGetEqInfo reports NA_EQ_MAX_SECTIONS, the number of entries and the device
 *   memory the stage holds.
 * NA_BatchSetStreamEq is REAL-TIME SAFE: host arithmetic on tables that exist.  At a moment when the stream runs cascade A (flat if it
 *   has none) it switches to a new cascade B over N = fadeSamples samples.  B starts from A's state: for i < min(S_A, S_B) section i
 *   of B copies the four values of section i of A; the other sections start at zero; a stream with no entry has an all-zero history.
 *   The k-th sample after the call is fl32(fl32(fl32(1 - w) * o_A) + fl32(w * o_B)) with w = (min(k, N-1) + 1) / N, the weight the
 *   other stages use; for w == 1 the sample is o_B itself.  N = 0 means B from k = 0: the classic coefficient change on kept state,
 *   with no doubled work.  During a fade both cascades run on the same input; after it A is dropped.  numSections = 0 (sections may
 *   be NULL) is the flat cascade: once it is the stream's only cascade the entry retires with its state.  The coefficients travel to
 *   the device once, with the first processing call after the set call; there is no coefficient interpolation.
 * NA_BatchGetStreamEq returns the section count of the target cascade and fills out[0 .. min(count, capacity)); < 0 on a bad id or when
 *   the stage is not enabled.  NA_BatchStreamEqFadeRemaining returns the samples left of the stream's EQ fade, 0 without one.
 * Rules (each fails with a message that names it, NA_GetLastError): the stage must be enabled; the stream must be live (a parked one
 *   fails with "... is parked"); numSections must lie in [0, 8]; every coefficient must be finite; every section must be stable,
 *   |a2| < 1 and |a1| < 1 + a2 (the message names the section index); fadeSamples must lie in [0, 1 << 20]; a set call while an EQ
 *   fade of that stream is running is refused; a broken batch refuses everything.  NA_BatchParkStream / NA_BatchRemoveStreams, and the
 *   park that ends a hand-over, make the stream flat at once and drop its state: an activated stream is flat.  The EQ is not part of a
 *   NA_BatchSaveStreams blob; NA_BatchLoadStreams leaves it alone.
 * The position k is kept per entry and advanced by whole calls.  While an entry exists -- a stream with a cascade, or one that fades
 * to flat -- a processing call behaves as it does with entries of the other stages: its launches run in order on one stream (no
 * half-batch chains, no resident launch), host buffers go through the library's device staging block, and it enqueues one table upload
 * from a ring of pinned tables plus ONE launch over the streams with an entry only, whatever n: no device or pinned allocation, no
 * stream or event creation, no unbounded wait.  The upload holds one small entry per stream with an entry and the coefficients of
 * the set calls since the last processing call -- not entries x sections.  With the last entry the free-running modes come back.
 * Not provided: the stage on NA_Multi* batches; the stage on the one-stream NeuralModel; more than 8 sections; coefficient
 * interpolation. */
#define NA_EQ_MAX_SECTIONS 8
typedef struct NA_EqSection { double b0, b1, b2, a1, a2; } NA_EqSection;   /* normalised, a0 == 1 */
typedef struct NA_EqInfo { int maxSections, numEntries; long long deviceBytes; } NA_EqInfo;
/* host arithmetic, no device.  kind: 0 low-pass, 1 high-pass, 2 low shelf, 3 high shelf, 4 peaking (RBJ cookbook, Q form) */
NA_EXTERN int NA_EqSectionFromDesign(int kind, double sampleRate, double freqHz, double q, double gainDb, NA_EqSection* out);
NA_EXTERN int NA_BatchEnableEqStage(NA_Batch* batch);                       /* set-up side, allocates, idempotent */
NA_EXTERN int NA_BatchGetEqInfo(NA_Batch* batch, NA_EqInfo* info);
NA_EXTERN int NA_BatchSetStreamEq(NA_Batch* batch, int stream, const NA_EqSection* sections, int numSections, int fadeSamples); /* 0 sections / NULL: flat */
NA_EXTERN int NA_BatchGetStreamEq(NA_Batch* batch, int stream, NA_EqSection* out, int capacity);   /* section count of the target; <0 bad id / not enabled */
NA_EXTERN int NA_BatchStreamEqFadeRemaining(NA_Batch* batch, int stream);
/* ---- the meter stage: per-stream level and gain-reduction meters ----
 * Every link of a session's chain -- model -> gate -> EQ -> cabinet -> reverb -> output gain -> mix (the delay stage, where enabled, sits between cabinet and reverb) -- can be set from the audio thread; this stage is what
 * can be READ from it: an input level and clip count, an output level, and what the gate did, per stream, without stopping the batch.
 * A host of the reference meters the buffers it holds; here the rows stay on the device.  A fifth per-stream stage, off unless enabled.
 * It never writes an audio row: with or without meters the samples out are the same bits.  A batch that enabled it and set no meter
 * launches exactly what it launched before.
 * Order of a processing call: the IN tap in front of everything, beside the gate detector -- it reads the input rows as the caller
 * passed them (in a resampling batch: the external-rate rows; input and output rows may be the same memory) -- then the models and the
 * other stages as before, then, behind the output stage, the OUT tap on the row the caller receives and the GATE tap on the gain the
 * gate stage applied to the same samples in this call.  The GATE tap reads 1 for every sample of a stream that was not an entry of the
 * gate stage in this call, or when the gate stage is not enabled.
 * Arithmetic.  This stage is not a recurrence: every quantity is a max, a min or an integer sum, hence exact, so a reading does not
 * depend on the order of evaluation, on how the signal is cut into calls, on alignment or on stride.  Positions count the samples the
 * caller sees since the meter was set; W = windowSamples; window k covers positions [kW, (k+1)W).  For each sample of a tap (clipLevel
 * is clipLevelIn on the IN tap, clipLevelOut on the OUT tap):
 *     x' = (x is NaN) ? 0 : min(|x|, 1e18f)
 *     q  = (unsigned) trunc(min(x', 8.0f) * 2^21)     (the product is exact; q <= 2^24)
 *     peak   = max(peak, x')        over the window      (exact; subnormals kept)
 *     energy = energy + q * q       over the window, unsigned 64-bit    (<= 2^63 for W <= 32768)
 *     overs  = overs + (x' >= clipLevel ? 1 : 0)   over the window
 *     peakHold   = max over every sample since the meter was set
 *     oversTotal = overs summed over every sample since the meter was set (64-bit)
 *   For the GATE tap, g the gain of the sample:
 *     gateGainMin  = min(g) over the window
 *     gateGainLast = g of the window's last sample
 *   The RMS of a window is sqrt(energy / W) / 2^21 -- for the host to compute, in whatever precision it likes.  The energy saturates at
 *   |x| = 8 (+18 dBFS) and reads 0 below 2^-21; the peak does not saturate there.  A reading is published when a window completes;
 *   peakHold and oversTotal of a reading run through the end of its window.  NA_MeterReading.windows is the number of completed
 *   windows: the reading describes window `windows - 1`.
 * NA_BatchEnableMeterStage is the set-up side (allocates; idempotent): a state per row, the stage's device + pinned tables and a
 *   device + pinned result block per table; later NA_BatchAddStreams / NA_BatchReserveStreams grow them.  Every call below fails
 *   ("meter stage not enabled (NA_BatchEnableMeterStage)") before it.  NA_BatchGetMeterInfo reports the number of meters and the device
 *   memory the stage holds.
 * NA_BatchSetStreamMeter is REAL-TIME SAFE: host arithmetic on tables that exist; no memset travels with it.
 *   The stream has no meter: the meter starts at the next sample, at position 0.
 *   The stream has a meter: it RESTARTS at position 0 with the new constants, holds and totals cleared; no reading is available until
 *     its first window completes, and nothing the earlier meter produced is read again.
 *   params == NULL: the meter goes at once (it touches no audio, so there is no tail).  On a stream without a meter it does nothing.
 *   windowSamples must lie in [32, 32768] (any integer, not only powers of two); clipLevelIn and clipLevelOut must be finite and > 0.
 *     Each failure names the field.
 * NA_BatchGetStreamMeter returns 1 and fills *out with the constants in effect, 0 when the stream has no meter, < 0 on a bad id or when
 *   the stage is not enabled.
 * NA_BatchReadStreamMeter is REAL-TIME SAFE: no wait, no allocation, no device call other than event queries.  It returns 1 and the
 *   newest reading that has ARRIVED on the host -- a processing call leaves its results in pinned memory behind its launches, and this
 *   call (like the start of every processing call) asks the events of those copies whether they are over --, 0 if the stream has no
 *   meter or no completed window has arrived yet, < 0 on a bad id, when the stage is not enabled, or on a broken batch.  Straight
 *   after a processing call the newest window may still be on its way: the reading says which window it is (`windows`).  After
 *   NA_BatchSynchronize everything has arrived.  Call it from the thread that drives the batch, like every other call.
 * Rules (each fails with a message that names it, NA_GetLastError): the stage must be enabled; the stream must be live (a parked one
 * fails with "... is parked"); a broken batch refuses everything.  NA_BatchParkStream / NA_BatchRemoveStreams, and the park that ends a
 * hand-over, drop the meter at once.  Meters are not part of a NA_BatchSaveStreams blob; NA_BatchLoadStreams leaves them alone.
 * While an entry exists -- a stream with a meter -- a processing call behaves as it does with entries of the other stages: its
 * launches run in order on one stream (no half-batch chains, no resident launch), host buffers go through the library's device staging
 * block, and it enqueues one table upload from a ring of pinned tables, two launches (IN; OUT + GATE) over the metered streams only and
 * one copy of entries * sizeof(record) into the pinned result block of the same ring slot, whatever n: no device or pinned allocation,
 * no stream or event creation, no unbounded wait.  With the last entry the free-running modes come back.
 * Not provided: the stage on NA_Multi* batches and on the one-stream NeuralModel; true-peak (oversampled) detection; loudness weighting. */
typedef struct NA_MeterParams  { int windowSamples; float clipLevelIn, clipLevelOut; } NA_MeterParams;
typedef struct NA_MeterTap     { unsigned long long energy, oversTotal; float peak, peakHold; unsigned int overs, reserved; } NA_MeterTap;
typedef struct NA_MeterReading { unsigned long long windows; NA_MeterTap in, out; float gateGainMin, gateGainLast; int windowSamples, reserved; } NA_MeterReading;
typedef struct NA_MeterInfo    { int numMeters; long long deviceBytes; } NA_MeterInfo;
NA_EXTERN int NA_BatchEnableMeterStage(NA_Batch* batch);                    /* set-up side, allocates, idempotent */
NA_EXTERN int NA_BatchGetMeterInfo(NA_Batch* batch, NA_MeterInfo* info);
NA_EXTERN int NA_BatchSetStreamMeter(NA_Batch* batch, int stream, const NA_MeterParams* params); /* params = NULL: the meter goes at once */
NA_EXTERN int NA_BatchGetStreamMeter(NA_Batch* batch, int stream, NA_MeterParams* out);  /* 1: filled; 0: no meter; < 0: bad id / not enabled */
NA_EXTERN int NA_BatchReadStreamMeter(NA_Batch* batch, int stream, NA_MeterReading* out); /* 1: filled; 0: nothing to read yet; < 0: bad id / not enabled / broken */
/* ---- the tuner stage: per-stream pitch readings ----
 * The tuner in front of the amp: every hopSamples it estimates the period of the row a stream takes in, from an autocorrelation of about
 * 85 ms of signal over several hundred lags -- on the order of a million multiply-adds an evaluation, times the sessions, times 20 - 50
 * evaluations a second: more than a host wants on its audio thread, and the dry rows are on the device already.  A sixth per-stream
 * stage, off unless enabled, last in the chain's order.  It never writes an audio row: with or without tuners the samples out are the
 * same bits.  A batch that enabled it and set no tuner launches exactly what it launched before.
 * Order of a processing call: everything the stage does runs in front of the models, behind the meter's IN tap -- it reads the input
 * rows as the caller passed them (in a resampling batch: the external-rate rows; input and output rows may be the same memory).
 * Arithmetic.  After one float multiply per sample everything is an integer, hence exact: a reading is the same bits however the
 * signal is cut into calls, at any alignment or stride.  Positions p = 0, 1, ... count the samples the caller sees on the stream's
 * input row since the set call (in a resampling batch: external-rate samples).  D = decimation, W = windowSamples, H = hopSamples;
 * W, minLag, maxLag, H and phase count decimated samples.
 *     c    = (x is NaN) ? 0 : min(max(x, -1.0f), 1.0f)
 *     q[p] = (int) trunc(c * 32767.0f)                      (one f32 product, then integers only)
 *     d[m] = q[mD] + q[mD+1] + ... + q[mD+D-1]   for m >= 0;   d[m] = 0 for m < 0        (|d| < 2^18)
 *     evaluation k = 0, 1, ... ends at m_k = phase + (k+1)*H - 1 and belongs to the call that holds position (m_k+1)*D - 1
 *     for t = 0 .. maxLag+1, signed / unsigned 64-bit:
 *         r[t] = sum over j = 0 .. W-1 of d[m_k - j] * d[m_k - j - t]                      (|r| < 2^47)
 *         e[t] = sum over j = 0 .. W-1 of d[m_k - j - t] * d[m_k - j - t]                  (e[0] = r[0])
 *     lag = 0 if e[0] < minEnergy
 *     z   = the smallest t in [1, maxLag+1] with r[t] <= 0;          none: lag = 0
 *     candidates: t in [max(minLag, z+1), maxLag] with r[t] > 0 and r[t] > r[t-1] and r[t] >= r[t+1];   none: lag = 0
 *     rmax = max of r[t] over the candidates
 *     lag  = the smallest candidate t with 1024 * r[t] >= thresholdQ10 * rmax              (< 2^57)
 *   A reading holds evaluations = k + 1, position = (m_k + 1) * D, lag (0: no pitch), decimation, e0 = e[0], and r[i], e[i] = r and e at
 *   lag - 1, lag, lag + 1 (all zero when lag = 0).  A call that holds several evaluation ends of a stream computes only the last of
 *   them; `evaluations` still counts them all: which evaluations are computed depends on the cut, the bits of evaluation k never do.
 * Limits (each refused with a message that names the field): decimation in [1, 8] (any integer); windowSamples in [32, 2048]; maxLag in
 *   [4, 1024]; minLag in [2, maxLag]; hopSamples in [16, 65536]; phase in [0, hopSamples); thresholdQ10 in [512, 1024].  minEnergy is any
 *   value; reserved is ignored.
 * NA_BatchEnableTunerStage is the set-up side (allocates; idempotent): an open group and a ring of 8192 decimated samples per row, the
 *   stage's device + pinned tables and a device + pinned result block per table; later NA_BatchAddStreams / NA_BatchReserveStreams grow
 *   them.  Every call below fails ("tuner stage not enabled (NA_BatchEnableTunerStage)") before it.  NA_BatchGetTunerInfo reports the
 *   number of tuners and the device memory the stage holds.
 * NA_BatchSetStreamTuner is REAL-TIME SAFE: host arithmetic on tables that exist; no memset travels with it.
 *   The stream has no tuner: the tuner starts at the next sample, at position 0.
 *   The stream has a tuner: it RESTARTS at position 0 with the new constants; no reading is available until its first evaluation has
 *     arrived, and nothing the earlier tuner took in or produced is read again.
 *   params == NULL: the tuner goes at once (it touches no audio, so there is no tail).  On a stream without a tuner it does nothing.
 * NA_BatchGetStreamTuner returns 1 and fills *out with the constants in effect, 0 when the stream has no tuner, < 0 on a bad id or when
 *   the stage is not enabled.
 * NA_BatchReadStreamTuner is REAL-TIME SAFE: no wait, no allocation, no device call other than event queries.  It returns 1 and the
 *   newest reading that has ARRIVED on the host -- a processing call that holds an evaluation end leaves its records in pinned memory
 *   behind its launches, and this call (like the start of every processing call) asks the events of those copies whether they are
 *   over --, 0 if the stream has no tuner or no evaluation has arrived yet, < 0 on a bad id, when the stage is not enabled, or on a
 *   broken batch.  The reading says which evaluation it is (`evaluations`, `position`).  After NA_BatchSynchronize everything has
 *   arrived.  Call it from the thread that drives the batch, like every other call.
 * Rules (each fails with a message that names it, NA_GetLastError): the stage must be enabled; the stream must be live (a parked one
 * fails with "... is parked"); a broken batch refuses everything.  NA_BatchParkStream / NA_BatchRemoveStreams, and the park that ends a
 * hand-over, drop the tuner at once.  Tuners are not part of a NA_BatchSaveStreams blob; NA_BatchLoadStreams leaves them alone.
 * While an entry exists -- a stream with a tuner -- a processing call behaves as it does with entries of the other stages: its
 * launches run in order on one stream (no half-batch chains, no resident launch), host buffers go through the library's device staging
 * block, and it enqueues one table upload from a ring of pinned tables and one append launch over the streams with a tuner per piece of
 * 4096 samples; a call that holds an evaluation end of an entry adds one evaluate launch over those entries only and one copy of
 * their records into the pinned result block of the same ring slot: no device or pinned allocation, no stream or event creation, no
 * unbounded wait.  With the last entry the free-running modes come back.
 * Host helpers (double precision, not part of the exact contract).  NA_TunerPitch: n_i = 2 r[i] / (e0 + e[i]) (0 on a zero denominator),
 *   den = n0 - 2 n1 + n2, off = den < 0 ? clamp(0.5 (n0 - n2) / den, +-1) : 0, hz = sampleRate / (D (lag + off)),
 *   clarity = n1 - 0.25 (n0 - n2) off; it returns 1, or 0 with hz = clarity = 0 when lag == 0, < 0 on a bad argument.
 *   NA_TunerParamsFromRange: D = the largest of 1..8 with sampleRate / (D highestHz) >= 16; maxLag = ceil(sampleRate / (D lowestHz)) + 2
 *   (above 1024 it fails with a message); minLag = max(2, floor(sampleRate / (D highestHz)) - 1); W = min(2048, max(32, 3 maxLag));
 *   H = max(16, round(sampleRate / (D evaluationsPerSecond))); phase 0, thresholdQ10 922, minEnergy = W (33 D)^2 (about -60 dBFS).
 *   It returns 0, or < 0 with a message.
 * Not provided: the stage on NA_Multi* batches and on the one-stream NeuralModel; polyphonic detection; a tap behind the gate; note
 * names. */
typedef struct NA_TunerParams  { int decimation, windowSamples, minLag, maxLag, hopSamples, phase, thresholdQ10, reserved;
                                 unsigned long long minEnergy; } NA_TunerParams;
typedef struct NA_TunerReading { unsigned long long evaluations; long long position; long long r[3];
                                 unsigned long long e0, e[3]; int lag, decimation; } NA_TunerReading;
typedef struct NA_TunerInfo    { int numTuners; long long deviceBytes; } NA_TunerInfo;
NA_EXTERN int NA_BatchEnableTunerStage(NA_Batch* batch);                                   /* set-up side, allocates, idempotent */
NA_EXTERN int NA_BatchGetTunerInfo(NA_Batch* batch, NA_TunerInfo* info);
NA_EXTERN int NA_BatchSetStreamTuner(NA_Batch* batch, int stream, const NA_TunerParams* params);  /* REAL-TIME SAFE; NULL: the tuner goes at once */
NA_EXTERN int NA_BatchGetStreamTuner(NA_Batch* batch, int stream, NA_TunerParams* out);    /* 1 / 0 / < 0 as the meter's */
NA_EXTERN int NA_BatchReadStreamTuner(NA_Batch* batch, int stream, NA_TunerReading* out);  /* REAL-TIME SAFE; 1 / 0 / < 0 as the meter's */
NA_EXTERN int NA_TunerParamsFromRange(double sampleRate, double lowestHz, double highestHz, double evaluationsPerSecond, NA_TunerParams* out);
NA_EXTERN int NA_TunerPitch(const NA_TunerReading* reading, double sampleRate, double* hz, double* clarity); /* host arithmetic; 0 when lag == 0 */
/* ---- the mix stage: per-session mix groups ----
 * Every stage above works on one row at a time.  A rig that runs two captures on one input, blended or panned left / right (dual amp),
 * an amp next to the dry DI (wet / dry), or wet / dry / wet needs rows to MEET, and the output rows never pass through host code that
 * could sum them: this is the place for it.  A seventh stage, off unless enabled, behind the output stage and in front of the meter
 * stage: a session's chain is model -> gate -> EQ -> cabinet -> output gain -> mix (the reverb stage, where enabled, sits between cabinet and output gain; the delay stage, where enabled, between cabinet and reverb), and the OUT tap of a meter on an output row of a
 * group reads the mixed row.  A batch that enabled it and has no group launches exactly what it launched before.
 * Model.  A mix group has M members, 1 <= M <= 8 (NA_MIX_MAX_MEMBERS).  A member is a pair (stream, tap); the tap is NA_MIX_TAP_OUT --
 * the stream's row as the output stage left it -- or NA_MIX_TAP_DRY -- the input row the caller passed for that stream in the same call.
 * The group has D outputs, 1 <= D <= M: the rows of its first D members, which must be OUT taps of distinct streams; the host reads
 * those rows as the session's mono or L / R signal.  A D x M gain matrix says what each output row becomes; rows that are not outputs
 * are never written.  A stream is named by at most one group, in one or both taps, and appears at most once per tap within a group.
 * Arithmetic.  Every operation is one separately rounded f32 operation, with no FMA contraction; fl() is that rounding.  The one
 * exception is the ramp weight, an f64 quotient rounded once to f32.  A group has one ramp (R, k) and two matrices g0 (from), g1 (to).
 *     The gain of cell (d, j) at the k-th sample after the set call is g1 for k >= R - 1.
 *     Before that it is fl(g0 + fl(fl(g1 - g0) * w)), with w = (float)((double)(k + 1) / (double)R).
 *     k is an integer advanced by whole calls and is never accumulated sample to sample: the samples do not depend on how the signal
 *     is cut into calls, on alignment or on stride.
 *     A set call during a ramp starts the new ramp from the gains of the last sample produced (the same function).
 *     A new group starts from the identity matrix -- output d takes member d at 1, everything else at 0 -- and ramps to the given
 *     matrix, so a group appears click-free.  R = 0 means the target from the next sample.
 *     For output d at a sample, the sum runs over the members j in member order whose gain at that sample is not exactly 0:
 *         acc = fl(g_dj * y_j) for the first such member
 *         acc = fl(acc + fl(g_dj * y_j)) for each further one
 *         if there is no such member, the output is +0.0f
 *     Hence a group at the identity matrix passes its rows bit for bit, and a NaN in a row whose gain is 0 stays where it is.
 *     Any finite gain is allowed, negatives included (a polarity flip is the point of a dual-amp blend).  Rows are not sanitised.
 *     The thread that owns a sample position reads that sample from all M sources before it writes any of the D outputs: an output
 *     row that is also a source of another output is read as the output stage left it.
 * NA_BatchEnableMixStage is the set-up side (allocates; idempotent): two 8 x 8 matrices and a row of drySamples floats for stashed input
 *   per row, and the stage's device + pinned tables; later NA_BatchAddStreams / NA_BatchReserveStreams grow them.  Every call below
 *   fails ("mix stage not enabled (NA_BatchEnableMixStage)") before it.  NA_BatchGetMixInfo reports maxMembers, the number of groups,
 *   drySamples (a power of two >= 2048) and the device memory the stage holds.
 * NA_BatchSetMixGroup is REAL-TIME SAFE: host arithmetic on tables that exist.  taps == NULL means all OUT; gains is
 *   [numOutputs][numMembers], row-major; rampSamples lies in [0, 1 << 20].  If the member list is exactly that of an existing group
 *   (same order, taps and numOutputs) the call is a gain change on the kept ramp state; otherwise every named stream must be in no
 *   group, and the call creates a new group.  The matrices travel once, behind the table of the next processing call.
 * NA_BatchClearMixGroup is REAL-TIME SAFE: the group that names `stream` goes at once; no group is not an error.  The click-free way to
 *   remove a group is to ramp to the identity and then clear, which is exact by the identity property.
 * NA_BatchGetStreamMix returns M and fills in the members (up to `capacity`), *numOutputs and -- when capacity >= M -- the target
 *   matrix [D][M]; 0 means no group; < 0 a bad id or the stage not enabled.  NA_BatchMixRampRemaining returns the samples the ramp of
 *   the stream's group still has to produce (0: none, or no group).
 * NA_MixGainsFromPan is host arithmetic, no device: equal power, level = 10^(levelDb / 20), left = level * cos((pan + 1) * pi / 4) and
 *   right = level * sin((pan + 1) * pi / 4), computed in double and rounded once; pan lies in [-1, 1]; pan = -1 gives exactly
 *   (level, 0) and pan = +1 exactly (0, level).  It returns 0, or < 0 with a message on a non-finite argument or |pan| > 1.
 * Rules (each fails with a message that names it, NA_GetLastError): the stage must be enabled; every named stream must be live (a
 * parked one fails with "... is parked"); numMembers in [1, 8] and numOutputs in [1, numMembers]; the outputs are OUT taps of
 * distinct streams; no (stream, tap) pair twice; a stream already in another group is refused with its id; every gain finite; the ramp
 * in range; a group with a DRY member is refused on a resampling batch -- the rows lag the input by the resampler's latency, and an
 * unaligned dry blend is a comb filter --, and NA_BatchSetResampling is refused while such a group exists; a broken batch refuses
 * everything.
 * NA_BatchParkStream / NA_BatchRemoveStreams, and the park that ends a hand-over, dissolve at once the group that names the stream: a
 * parked stream carries nothing over.  Hand-over recipe: at the call that issues NA_BatchHandover(from, to, ...), clear the group and
 * set it again with `to` in the place of `from`, at the same gains and with rampSamples = 0.  During the fade row `to` carries the
 * output stage's cross-fade, so the mix stays continuous, and nothing happens to it when `from` is parked.  Groups are not part of a
 * NA_BatchSaveStreams blob.
 * While a group exists a processing call behaves as it does with entries of the other stages: its launches run in order on one stream
 * (no half-batch chains, no resident launch), host buffers go through the library's device staging block, and it enqueues one table
 * upload from a ring of pinned tables and ONE launch over the groups, whatever n -- and, while some group has a DRY member, one small
 * launch in front of the models that keeps those members' input rows (input and output rows may be the same memory): no device or
 * pinned allocation, no stream or event creation, no unbounded wait.  The one exception: the first call with a DRY member that is
 * longer than drySamples grows the stash block first, like any first use of a longer buffer.  With the last group the free-running
 * modes come back.
 * Not provided: the stage on NA_Multi* batches and on the one-stream NeuralModel; latency-compensated dry taps on resampling batches. */
#define NA_MIX_MAX_MEMBERS 8
#define NA_MIX_TAP_OUT 0
#define NA_MIX_TAP_DRY 1
typedef struct NA_MixInfo { int maxMembers, numGroups, drySamples; long long deviceBytes; } NA_MixInfo;
NA_EXTERN int NA_BatchEnableMixStage(NA_Batch* batch);                                     /* set-up side, allocates, idempotent */
NA_EXTERN int NA_BatchGetMixInfo(NA_Batch* batch, NA_MixInfo* info);
NA_EXTERN int NA_BatchSetMixGroup(NA_Batch* batch, const int* streams, const int* taps, int numMembers, int numOutputs, const float* gains,
                                  int rampSamples);                                        /* REAL-TIME SAFE */
NA_EXTERN int NA_BatchClearMixGroup(NA_Batch* batch, int stream);                          /* REAL-TIME SAFE */
NA_EXTERN int NA_BatchGetStreamMix(NA_Batch* batch, int stream, int* streams, int* taps, int capacity, int* numOutputs, float* gains);
NA_EXTERN int NA_BatchMixRampRemaining(NA_Batch* batch, int stream);
NA_EXTERN int NA_MixGainsFromPan(double levelDb, double pan, float* left, float* right);   /* host arithmetic, no device */
NA_EXTERN int NA_BatchNumStreams(NA_Batch* batch);     /* rows of the [streams][n] arrays, retired and parked ids included */
NA_EXTERN int NA_BatchNumLiveStreams(NA_Batch* batch);
NA_EXTERN int NA_BatchIsLive(NA_Batch* batch, int stream);
NA_EXTERN int NA_BatchSetQuality(NA_Batch* batch, int stream, float quality);
NA_EXTERN int NA_BatchGetActiveSubModel(NA_Batch* batch, int stream);
/* 1 when NA_BatchSetQuality(stream, quality) costs the next NA_BatchProcess* call no allocation / synchronisation / prewarm */
NA_EXTERN int NA_BatchIsQualityChangeRealtimeSafe(NA_Batch* batch, int stream, float quality);
NA_EXTERN int NA_BatchPrewarm(NA_Batch* batch, int stream); /* stream < 0: all */
/* host pointers, layout [streams][n]; synchronous */
NA_EXTERN int NA_BatchProcess(NA_Batch* batch, const float* in, float* out, size_t n);
/* Optional, for hosts that reuse their buffers: a registered block (pinned and mapped: hipHostRegister) is read / written by the kernels
 * as it is when NA_BatchProcess is handed pointers inside it -- no staging copies (1024 x 128: 81 -> ~62 us per call).  Register once,
 * outside the audio path (it pins pages: milliseconds); the block must stay allocated until NA_UnregisterHostBuffer.  0 on success. */
NA_EXTERN int NA_RegisterHostBuffer(void* ptr, size_t bytes);
NA_EXTERN int NA_UnregisterHostBuffer(void* ptr);
/* Pipelined host-buffer interface: NA_BatchSubmit copies `in` ([streams][n]) and enqueues upload, kernels and download, returning a
 * ticket (>= 0; up to 3 may be in flight); NA_BatchCollect blocks until that buffer is done and copies its [streams][n] result to
 * `out`.  Uploads / downloads of neighbouring buffers overlap the kernels.  Buffers are processed in submission order. */
NA_EXTERN int NA_BatchSubmit(NA_Batch* batch, const float* in, size_t n);
NA_EXTERN int NA_BatchCollect(NA_Batch* batch, int ticket, float* out);
/* Zero-copy variants: NA_BatchNextInput returns the pinned [streams][n] staging buffer of the next submission -- fill it, then call
 * NA_BatchSubmit(batch, NULL, n); NA_BatchCollect(batch, ticket, NULL) only waits, and NA_BatchOutputView(batch, ticket) is the pinned
 * result, valid until that slot is submitted again (3 submissions later). */
NA_EXTERN float* NA_BatchNextInput(NA_Batch* batch, size_t n);
NA_EXTERN const float* NA_BatchOutputView(NA_Batch* batch, int ticket);
/* DEVICE pointers, row s = stream s, rows `stride` floats apart.  Two contracts, by who owns the stream:
 *
 * (a) the batch runs on a stream of the CALLER (NA_BatchCreate with a stream handle), or the caller has fetched the batch's own stream
 *     (NA_BatchGetHipStream): every launch is ordered on that stream, like any HIP kernel launch -- a producer kernel enqueued on it
 *     before the call and a consumer enqueued after it need no other synchronisation, and the call may be made from a device-side
 *     pipeline without any host wait.
 *
 * (b) the batch created its own stream (hipStream == NULL) and nobody has fetched it: the library schedules the buffer itself -- as
 *     two free-running launches of half the streams each on internal streams, or, where NA_BatchSetResidentLaunch asked for it, for
 *     large A1 Standard batches as a command to ONE resident launch that stays on the chip and walks consecutive buffers
 *     (csrc/gpu_batch_chains.cpp) -- none of which is ordered against any stream the caller knows.  The contract is then a HOST-side one:
 *       - the input rows must be COMPLETE in device memory when NA_BatchProcessDevice is called (synchronise their producer first:
 *         hipStreamSynchronize / hipEventSynchronize on its stream) and must stay untouched until the step's outputs are valid;
 *       - the output rows are valid after NA_BatchWaitOutputs (cheap: the resident launch stays up) or NA_BatchSynchronize (everything
 *         of the batch is idle, the resident launch has left the chip);
 *       - a caller that re-uses ONE output buffer for consecutive steps can only ever read the rows of the last step it waited for: give
 *         every step that is in flight its own output rows (up to 63 steps may be in flight; the call blocks beyond that);
 *       - a device-side producer / consumer that must not wait on the host cannot use (b): create the batch on its stream, contract (a).
 *     Inside the resident launch the rows are read and written at system scope, so a producer that ran on another stream / XCD between
 *     two steps is seen without a kernel boundary (tests/test_gpu_resident.py: a producer kernel on a foreign stream rewrites the same
 *     input buffer before every step). */
NA_EXTERN int NA_BatchProcessDevice(NA_Batch* batch, const float* dIn, float* dOut, size_t n, long inStride, long outStride);
/* every buffer handed to NA_BatchProcessDevice so far has been processed: its output rows are valid (host-side wait; contract (b)) */
NA_EXTERN int NA_BatchWaitOutputs(NA_Batch* batch);
NA_EXTERN int NA_BatchSynchronize(NA_Batch* batch);
/* Bounded waits.  Process is called from a real-time thread that must get its call back (NeuralAudio/NeuralModel.h:127): every host-side
 * wait of the processing entry points -- NA_BatchProcess, NA_BatchCollect, NA_BatchWaitOutputs, NA_BatchSynchronize, the timing marks,
 * the legacy Process / NA_ProcessChecked (a batch of one) -- gives up after a wall-clock limit: default 2000 ms, environment
 * NA_WAIT_LIMIT_MS for every batch of the process, NA_BatchSetWaitLimitMs for one batch (<= 0: wait without a limit).  A wait that runs
 * into the limit marks the batch BROKEN: the call returns non-zero with the reason in NA_GetLastError(), NA_BatchProcess / Process
 * hand back silence (zeros), and every later call on the batch fails at once without touching the device (the stream states are no
 * longer what the caller thinks they are).  A broken batch can only be destroyed; NA_BatchDestroy gives the device one more limit to
 * come back and otherwise leaves the device allocations alone instead of waiting in hipFree.  NA_BatchIsBroken: 1 / 0. */
NA_EXTERN int NA_BatchSetWaitLimitMs(NA_Batch* batch, double milliseconds);
NA_EXTERN double NA_BatchGetWaitLimitMs(NA_Batch* batch);
NA_EXTERN int NA_BatchIsBroken(NA_Batch* batch);
/* The batch's HIP stream.  Fetching it switches a batch that created its own stream from contract (b) to contract (a) for good: the
   internal launches are joined, and from then on every launch is ordered on this stream. */
NA_EXTERN void* NA_BatchGetHipStream(NA_Batch* batch);
/* Timing marks for benchmarks: HIP events recorded on EVERY stream the batch launches kernels on.  NA_BatchMarkTime(b, 0) ... launches ...
   NA_BatchMarkTime(b, 1); NA_BatchElapsedMs waits for the second mark and returns the longest mark-to-mark span over those streams (< 0: error). */
NA_EXTERN int NA_BatchMarkTime(NA_Batch* batch, int which);
NA_EXTERN int NA_BatchWaitMarks(NA_Batch* batch); /* polls until the second marks are reached on every stream */
NA_EXTERN float NA_BatchElapsedMs(NA_Batch* batch);
/* 1: the last NA_BatchProcessDevice call ran as two half-batch launches (see NA_BatchGetHipStream) */
NA_EXTERN int NA_BatchUsesHalfLaunches(NA_Batch* batch);
/* Opt-in (off unless the environment says NA_RESIDENT=1): device-pointer buffers of a batch on its own stream whose streams are >= 512
   A1 Standard models become commands to one resident launch (contract (b) above).  Measured on MI355X: per-buffer
   latency of a lone buffer 41 - 44 us instead of 43 - 48, sustained throughput 38.5 - 39.7 us per 1024 x 128 step instead of 36.6 -- the
   chip is power-limited on this kernel, so keeping every slot busy buys clock throttling, not throughput.  0 on success. */
NA_EXTERN int NA_BatchSetResidentLaunch(NA_Batch* batch, int on);
/* 1: the last NA_BatchProcessDevice call was a command to the resident launch */
NA_EXTERN int NA_BatchUsesResidentLaunch(NA_Batch* batch);
/* roofline bookkeeping (stream-weighted means): compulsory HBM bytes and multiply-accumulates per sample */
NA_EXTERN double NA_BatchAlgorithmicBytesPerSample(NA_Batch* batch, int blockFrames);
NA_EXTERN double NA_BatchMacsPerSample(NA_Batch* batch);
NA_EXTERN double NA_BatchStateBytes(NA_Batch* batch);
/* > 1 when the stream of a narrow static WaveNet model runs packed with others of its model into one kernel-level stream (0: bad argument) */
NA_EXTERN int NA_BatchStreamPackFactor(NA_Batch* batch, int stream);
/* the kernel that runs the stream (its rocprof name without template arguments; static string, "" on a bad argument) */
NA_EXTERN const char* NA_BatchStreamKernelName(NA_Batch* batch, int stream);
/* ---- stream snapshots: save and restore of live stream state (csrc/stream_snapshot.h) ------------
 * A snapshot is one self-contained, relocatable blob per stream: the history of every conv layer / the recurrent state of every submodel
 * plus quality, active submodel and prewarmed bits, behind a versioned header with a fingerprint of the model (architecture + weights).
 * It loads into any stream created from the same model file -- in another batch, on another device, in another process, on another kernel
 * family -- and the stream then continues where the saved one stopped: bit for bit where the same kernel runs both, else to the kernels'
 * usual tolerance.  Moving a session between GPUs, parking and resuming it, consolidating batches, rewinding for an A/B comparison.
 *
 * Both calls first wait for everything of the batch that is in flight (like NA_BatchRemoveStreams): NOT real-time safe, call them
 * between buffers, never from the audio callback.  A broken batch refuses both.  Cost: one device launch per model of the listed
 * streams and one device <-> host copy per call, however many streams the call names. */
/* bytes NA_BatchSaveStreams writes for this stream (host arithmetic; no device work); negative on a bad argument */
NA_EXTERN long long NA_BatchStreamSnapshotBytes(NA_Batch* batch, int stream);
/* the same from a model alone, without a batch or a device */
NA_EXTERN long long NA_ModelSnapshotBytes(NeuralModel* model);
/* fingerprint a snapshot of this model carries (host arithmetic): the same for every load of one file whatever the math mode or kernel */
NA_EXTERN unsigned long long NA_ModelSnapshotFingerprint(NeuralModel* model);
/* blobs of streams[0..count) back to back into buf; *written = total bytes.  Non-zero (and *written = bytes needed, nothing written to
 * buf) if capacity is short.  Saving changes nothing: the streams continue as if it had not been called. */
NA_EXTERN int NA_BatchSaveStreams(NA_Batch* batch, const int* streams, int count, void* buf, size_t capacity, size_t* written);
/* the inverse: blob i goes to streams[i] (each id at most once).  All-or-nothing: every blob is checked first -- magic, version, size,
 * model fingerprint against the destination stream's model, submodel count -- and on any mismatch the call returns non-zero with the
 * reason in NA_GetLastError() and no stream has changed.  The destination keeps its own composite load mode. */
NA_EXTERN int NA_BatchLoadStreams(NA_Batch* batch, const int* streams, int count, const void* buf, size_t bytes);
/* the one-stream NeuralModel of the legacy API is a batch of one (call them from the thread that calls Process) */
NA_EXTERN int NA_SaveModelState(NeuralModel* model, void* buf, size_t capacity, size_t* written);
NA_EXTERN int NA_LoadModelState(NeuralModel* model, const void* buf, size_t bytes);

/* ---- multi-GPU host: one batch + one host thread + one HIP stream per device ------------------------------------------------
 * The GLOBAL stream list (order of the NA_MultiAddStreams calls: sort it by architecture) is cut into contiguous ranges of near-equal
 * cost, one per entry of `devices` (an index may repeat).  Streams are independent (the reference runs one NeuralModel per stream,
 * NeuralModel.h:127), so there is no data-path collective: every shard uploads, processes and downloads its own rows of the caller's
 * [streams][n] arrays. */
typedef struct NA_MultiBatch NA_MultiBatch;
NA_EXTERN NA_MultiBatch* NA_MultiCreate(const int* devices, int numDevices);
NA_EXTERN void NA_MultiDestroy(NA_MultiBatch* multi);
NA_EXTERN int NA_MultiAddStreams(NA_MultiBatch* multi, NeuralModel* model, float quality, int count, int doPrewarm); /* first global id */
NA_EXTERN int NA_MultiCommit(NA_MultiBatch* multi);   /* shard + create the device state (implied by the first Process / Submit) */
NA_EXTERN int NA_MultiNumStreams(NA_MultiBatch* multi);
NA_EXTERN int NA_MultiNumShards(NA_MultiBatch* multi);
NA_EXTERN int NA_MultiShardRange(NA_MultiBatch* multi, int shard, int* begin, int* end, int* device);
NA_EXTERN int NA_MultiProcess(NA_MultiBatch* multi, const float* in, float* out, size_t n);   /* host [streams][n]; synchronous */
NA_EXTERN int NA_MultiSubmit(NA_MultiBatch* multi, const float* in, size_t n);                /* pipelined, like NA_BatchSubmit */
NA_EXTERN int NA_MultiCollect(NA_MultiBatch* multi, int ticket, float* out);
NA_EXTERN int NA_MultiSetQuality(NA_MultiBatch* multi, int stream, float quality);
/* Fan-out / fan-in between the devices of a multi batch; call before NA_MultiCommit.  0 (default): host rows -- every shard uploads its
 * weights from the host and downloads its rows into the caller's array, no GPU talks to another.  1: RCCL over xGMI (librccl.so is
 * loaded with dlopen at this point; devices must be distinct) -- a model's weight images are replicated from the first shard that holds
 * it (ncclSend / ncclRecv), NA_MultiProcess gathers every shard's output rows into a [streams][n] device buffer on every GPU (an
 * all-gather of unequal parts) and serves the host array from shard 0 in one download; NA_MultiGatheredOutput(multi, shard) is that
 * buffer on the shard's GPU (valid until the next NA_MultiProcess).  The kernels' data path has no collective either way. */
NA_EXTERN int NA_MultiSetFanIn(NA_MultiBatch* multi, int mode);
NA_EXTERN const float* NA_MultiGatheredOutput(NA_MultiBatch* multi, int shard);
/* 1 when librccl.so loads and exports every entry point this library binds (no GPU needed), else 0 with NA_GetLastError().  The first
 * call is the dlopen (seconds on a cold page cache: measured 4.9 s): a set-up call, never one for the audio thread. */
NA_EXTERN int NA_RcclAvailable(void);
/* the partition itself: bounds[0 .. parts] of contiguous ranges of items [0, n) with near-equal total cost (every range keeps at least
 * one item while items remain).  One-process-per-GPU hosts (bench.py over torch.distributed / RCCL) call it with their rank. */
NA_EXTERN int NA_ShardByCost(const double* cost, int n, int parts, int* bounds);
/* relative cost of one stream of `model` at `quality` (what the sharder balances): estimated microseconds per 1024 streams x 128 frames */
NA_EXTERN double NA_ModelStreamCost(NeuralModel* model, float quality);

/* Host side only (no GPU needed): the kernel family a batch of `streams` streams of `model` would run on -- "f16-split", "frame" (f32),
 * "generic" (wide arrays) or "recurrent" -- with the facts behind the choice: the input limit of the f16-split range proof, whether the
 * proof holds (every value stays inside the f16 range for inputs within the limit, limit >= 8), whether the weights fit the operand
 * format, and the stream-packing factor.  A WaveNet model that fails the proof runs on the f32 frame kernel.  0 on success. */
NA_EXTERN int NA_ModelKernelInfo(NeuralModel* model, float quality, int streams, char* kernelBuf, int bufSize, float* inputLimit, int* rangeProven,
	int* weightsOk, int* packFactor);

/* Range contract of the kernel that runs the stream: input samples beyond +-limit are clamped, NaN reads as silence.  +inf for the f32
 * kernels (they follow the reference's f32 chain at any amplitude); a per-model bound <= 32752 for the f16-split WaveNet kernels, whose
 * values carry an f16 exponent -- far above any audio level (0 on a bad argument). */
NA_EXTERN float NA_BatchStreamInputLimit(NA_Batch* batch, int stream);
/* Models the f16-split kernels run WITHOUT a static range proof (LeakyReLU: the official A2 shapes) saturate a value that leaves the f16
 * range instead of overflowing, and count it: the number of (wave, block) pairs of this stream in which that happened since its last
 * reset / prewarm.  0 = the stream's output is the reference's to the usual tolerance; > 0 = some block was computed with clamped values
 * (the stream recovers one receptive field later).  Always 0 for proven models and the f32 kernels.  Synchronises the batch stream: a
 * diagnostic, not for the audio path.  Negative on a bad argument. */
NA_EXTERN int NA_BatchStreamRangeEvents(NA_Batch* batch, int stream);

/* ---- offline rendering of long signals (csrc/offline_render.cpp) --------------------------------------------------
 * NA_RenderOffline renders every job's whole signal through its model and writes exactly what a FRESH instance of that model (same
 * loader settings: quality, math modes, external sample rate) would output after Prewarm() through Process() over the whole signal.
 * It never reads or writes the stream state of the NeuralModel passed in: it builds a temporary batch from it (as NA_BatchAddStreams).
 *
 * WaveNet models have no recurrence -- output t depends only on the inputs in [t - H, t], H the summed history of the stream's rings --
 * so a long signal is cut into segments that run as the streams of one batch, every segment after the first starting `lead` >= H
 * samples early (rounded up to 128) and keeping only what follows its lead-in.  Its output is the sequential run's bit for bit where the
 * segment batch runs the stream on the same kernel as a batch of one (NA_BatchStreamKernelName), else to the kernels' usual tolerance.
 * Recurrent models (LSTM, GRU, keras stacks) cannot be cut exactly: each recurrent job is one stream run sequentially from its prewarmed
 * state, and the gain comes only from rendering many jobs in one call.  Jobs of one call share one batch on the device of job 0's
 * model; all models must be on that device.
 *
 * Host pointers, pageable or registered; a job's input and output must not overlap.  Synchronous: every wait is bounded by the wait
 * limit (NA_BatchSetWaitLimitMs; waitLimitMs); a failure returns non-zero with the reason in NA_GetLastError().  Device memory: about
 * 3 x 4 bytes per sample of a pass's segment rows plus the batch's stream state; a signal longer than maxSamplesPerPass is rendered in
 * several passes. */
typedef struct NA_RenderJob
{
	NeuralModel* model;
	float quality;      /* the submodel of a slimmable model (ignored otherwise) */
	const float* input;
	float* output;
	size_t numSamples;
} NA_RenderJob;
typedef struct NA_RenderOptions
{
	size_t segmentSamples;    /* kept samples per segment (0: the planner's choice) */
	size_t maxSamplesPerPass; /* bound of a pass's segment rows in samples, i.e. of its device buffers (0: 64 Mi) */
	double waitLimitMs;       /* 0: the batch default (NA_WAIT_LIMIT_MS, 2000 ms) */
} NA_RenderOptions;
typedef struct NA_RenderPlanInfo
{
	long long segments;   /* over all jobs (a recurrent job: 1) */
	int lead;             /* lead-in of every segment after the first (a multiple of 128; 0 without WaveNet jobs) */
	long long segmentSamples; /* samples a segment after the first keeps */
	long long rowSamples; /* samples every stream of the segment batch processes per pass (lead + segmentSamples) */
	int passes;
	int streams;          /* streams of the segment batch */
	double estimatedMs;   /* the planner's estimate of the device time */
	char kernel[64];      /* with a device: NA_BatchStreamKernelName of job 0's first segment; else "" */
} NA_RenderPlanInfo;
/* opts may be NULL (all defaults).  0 on success. */
NA_EXTERN int NA_RenderOffline(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts);
/* the plan of NA_RenderOffline without running it (no device needed; with one it also builds the segment batch for info->kernel) */
NA_EXTERN int NA_RenderPlan(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts, NA_RenderPlanInfo* info);

/* ---- batch resampling: hosts whose sample rate is not the model's (csrc/resample.h) -------------
 * Every model has one sample rate; the loader serves whole multiples of it by multiplying the dilations (NA_SetExternalSampleRate), and
 * every other external rate -- 44.1 kHz against a 48 kHz capture -- would run the model at the wrong rate.  A resampling batch converts
 * on the device: ONE clock domain per batch (one external rate Fe, one model rate Fm, one phase for all its streams; a server keeps one
 * batch per client rate).  With Fc = lcm(Fe, Fm), te = Fc / Fe, tm = Fc / Fm, one Kaiser-windowed sinc prototype at Fc of length
 * K = 48 * max(te, tm) + 1 (pass band to 16 / 22.05 of the lower Nyquist frequency, stop band from that Nyquist frequency, 100 dB)
 * serves both directions.  The model only ever runs whole multiples of the block quantum q (1, 32, 64 or 128 frames; 0 = the default,
 * 32): after E external samples it has run P(E) = floor(J(E) / q) * q frames, J(E) = floor((E - 1) * te / tm) + 1 -- with q = 32 and
 * 128-sample calls at 44.1 kHz the model sees 128, 128, 160, ... frames and never a remainder block.  The output is delayed by a FIXED
 * whole number of external samples, latencySamples = (48 * max(te, tm) + (q - 1) * tm + pad) / te whatever the call lengths (48 / 77 /
 * 165 samples at 44.1 kHz for q = 1 / 32 / 128), and it is bit for bit independent of how the signal is cut into calls (any n >= 1).
 * A NaN input sample reads as silence before the filter.  Pairs whose te or tm exceeds 640 are refused. */
typedef struct NA_ResampleInfo {
	int externalRate, modelRate;
	int ticksExternal, ticksModel;   /* te, tm */
	int tapsUp, tapsDown;            /* taps per output sample of each stage */
	int quantum;                     /* q in effect */
	int latencySamples;              /* external samples; 0 when the rates are equal */
	int prototypeLength;             /* K */
} NA_ResampleInfo;
/* host arithmetic only, no device: the plan for a rate pair (quantum 0: the default); non-zero + NA_GetLastError() if refused */
NA_EXTERN int NA_ResamplePlan(int externalRate, int modelRate, int quantum, NA_ResampleInfo* info);
/* the f32 prototype of that plan into buf[capacity] (as many as fit); returns K, negative if the pair is refused */
NA_EXTERN int NA_ResamplePrototype(int externalRate, int modelRate, float* buf, int capacity);
/* model frames P(E) run after E external samples (host arithmetic; what a host needs to size anything by); negative if refused */
NA_EXTERN long long NA_ResampleModelFrames(int externalRate, int modelRate, int quantum, long long externalSamples);
/* Set-up call, before the first NA_BatchAddStreams of the batch (refused afterwards and on a broken batch): every n of the processing
 * entry points -- NA_BatchProcess (pageable and registered blocks), NA_BatchProcessDevice (n and strides), NA_BatchSubmit / Collect /
 * NextInput / OutputView -- now counts EXTERNAL samples per row.  maxFrames: the largest n the host will pass (device buffers are sized
 * here; a larger n later grows them -- not real-time safe, like any first use of a longer buffer; calls beyond 2048 samples run in
 * pieces).  externalRate == modelRate is accepted and means "no resampling": the batch behaves bit for bit as without the call and
 * reports latency 0.  NA_BatchAddStreams then refuses a model whose model-side rate (NA_GetModelProcessRate) is not modelRate.
 * A resampling batch orders its work on the batch stream -- up kernel, model launches, down kernel -- under either contract of
 * NA_BatchProcessDevice: it does not use the half-batch launches or the resident launch (NA_BatchUsesHalfLaunches / UsesResidentLaunch
 * answer 0; NA_BatchSetResidentLaunch is accepted and has no effect).  New, recycled and prewarmed streams (NA_BatchAddStreams,
 * NA_BatchPrewarm) start from zero filter histories at the batch's current phase; NA_BatchSetQuality keeps them.  Timing marks, bounded
 * waits and the broken-batch rules are those of every batch.  Not provided: NA_BatchSaveStreams / NA_BatchLoadStreams on a resampling
 * batch (they fail and say so: the v1 blob has no place for the filter histories, and the phase belongs to the batch, not the stream),
 * per-stream rates inside one batch.  Offline rendering and the multi-GPU host at an external rate: NA_RenderOfflineAtRate and
 * NA_MultiSetResampling below. */
NA_EXTERN int NA_BatchSetResampling(NA_Batch* batch, int externalRate, int modelRate, int quantum, int maxFrames);
/* the plan in effect; non-zero if NA_BatchSetResampling was never called on the batch */
NA_EXTERN int NA_BatchGetResampleInfo(NA_Batch* batch, NA_ResampleInfo* info);
/* loader opt-in for the one-stream NeuralModel (a batch of one): with on != 0, a model created while the loader's external rate is
 * neither the model's rate nor a whole multiple of it resamples inside Process / NA_ProcessChecked (default quantum; a refused rate
 * pair fails the load).  Default 0: today's behaviour, which is the reference's. */
NA_EXTERN void NA_SetResampleToExternalRate(NeuralModelLoader* loader, int on);
NA_EXTERN int NA_GetProcessLatencySamples(NeuralModel* model);   /* external samples; 0 unless the model resamples */
/* the model-side rate of this model as loaded: the file's rate times the integer oversampling factor the loader APPLIED -- what to
 * pass as modelRate (host arithmetic).  0 if the file's rate is not a whole number. */
NA_EXTERN int NA_GetModelProcessRate(NeuralModel* model);
/* ---- offline rendering at an external rate: files at 44.1 kHz through 48 kHz captures (csrc/offline_render.cpp) ------
 * As NA_RenderOffline, but every job's input, output and numSamples are at externalRate, whatever rate its model runs at.  Job i's
 * model rate is Fm = NA_GetModelProcessRate(job.model) and its plan NA_ResamplePlan(externalRate, Fm, quantum 1); jobs of one call may
 * have different model rates.  With L = latencySamples, N = numSamples and M = NA_ResampleModelFrames(externalRate, Fm, 1, N + L) model
 * frames: out[k] = s[k + L] for k in [0, N), s what a fresh resampling batch of one prewarmed stream (NA_BatchSetResampling(externalRate,
 * Fm, quantum 1), same loader settings) returns when fed x[0 .. N) followed by L zeros.  The result is therefore LATENCY-COMPENSATED --
 * out[k] lines up with x[k] -- and the filter's tail is rendered instead of being cut off.  It equals that streaming batch bit for bit
 * where the segment batch and the batch of one run the stream on the same kernel (NA_BatchStreamKernelName; NA_RenderOffline's own
 * rule); the two resampling stages are bit-identical to the streaming stages in every case (one shared sum per output sample).  A job
 * whose model runs at externalRate is rendered exactly as NA_RenderOffline renders it (L = 0).  NaN input reads as silence, +-inf as the
 * largest finite value.  The model's own loader opt-in (NA_SetResampleToExternalRate) is ignored: the call builds a temporary batch
 * from the loaded model, as NA_RenderOffline does.  Recurrent jobs stay one sequential stream each, over their M frames.
 *
 * Per job: x is uploaded whole, an up kernel makes the model-rate signal u[0 .. M) in device memory, the segment machinery of
 * NA_RenderOffline renders u to v there, a down kernel makes out, which is downloaded whole.  opts->segmentSamples,
 * opts->maxSamplesPerPass and every field of NA_RenderPlanInfo count MODEL-RATE frames.  Device memory: NA_RenderOffline's (3 x 4
 * bytes per frame of a pass's segment rows, which maxSamplesPerPass keeps bounding, plus the stream state) plus whole-signal buffers of
 * 8 N + 8 M bytes per job (8 M for a job that does not resample) and the coefficient tables (31 + 34 KB at 44.1 / 48 kHz); the call
 * fails with a message naming the size when they cannot be allocated.  Every wait is bounded as in NA_RenderOffline.
 * The whole call fails BEFORE any device work on externalRate <= 0, on a pair NA_ResamplePlan refuses (a reduced term above 640), on a
 * job without a model and on overlapping buffers. */
NA_EXTERN int NA_RenderOfflineAtRate(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts, int externalRate);
/* the plan of NA_RenderOfflineAtRate without running it (no device needed): NA_RenderPlan of jobs of M model-rate frames each;
 * resample: the resampling plan of job 0's rate pair, may be NULL */
NA_EXTERN int NA_RenderPlanAtRate(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts, int externalRate,
                                  NA_RenderPlanInfo* info, NA_ResampleInfo* resample);
/* ---- multi-GPU host at an external rate ----
 * Before NA_MultiCommit (refused afterwards, on a refused pair and on a bad quantum; arguments as NA_BatchSetResampling): every
 * shard's batch becomes a resampling batch of this plan, and every n of NA_MultiProcess, NA_MultiSubmit and NA_MultiCollect counts
 * EXTERNAL samples.  All shards share one phase, because they are always called with the same n; the library compares their sample
 * counters after every call and refuses further work on the multi batch if they ever disagree.  A model whose process rate is not
 * modelRate fails NA_MultiAddStreams (and this call, if it is already on the list) with NA_BatchAddStreams' message.  Both fan-in modes
 * work: with RCCL fan-in (NA_MultiSetFanIn 1) the gathered buffer is [streams][n] in external samples. */
NA_EXTERN int NA_MultiSetResampling(NA_MultiBatch* multi, int externalRate, int modelRate, int quantum, int maxFrames);
/* the plan in effect; non-zero if NA_MultiSetResampling was never called on the multi batch */
NA_EXTERN int NA_MultiGetResampleInfo(NA_MultiBatch* multi, NA_ResampleInfo* info);
#ifndef NA_RELEASE
/* ---- test / tuning hooks: exported by the test build only (csrc/Makefile default target; what tests/ loads).  The release library
 * (make RELEASE=1 -> dist/libNeuralAudioCAPI.so: -DNA_RELEASE -DNA_NO_TUNING, no loopback RCCL table) has none of the NA_Debug* symbols
 * and reads no tuning environment variable. ---- */
/* NAMIsA2 (bit 0) / NAMIsA2Standard (bit 1) of a .nam document (NeuralModel.cpp:159-168, 188-317); negative on a parse error */
NA_EXTERN int NA_DebugClassifyNam(const char* jsonText);
/* stream packing, host side only: pack factor of the model in a large batch (1: none); flat weights of the packed virtual model into
 * out[capacity] when given; returns their count (0: model does not pack), -1 on failure */
NA_EXTERN int NA_DebugPackedWeights(NeuralModel* model, int* packFactor, float* out, int capacity);
/* the f16-split kernels' plan of a WaveNet as an unpacked stream runs it, host side only: 16 ints per stage (WnSplitStage) into
 * stages[stageCapacity], the A-operand image (f16 bit patterns) into wsplit[wsplitCapacity], its length into *wsplitCount; returns the
 * stage count, -1 on failure */
NA_EXTERN int NA_DebugSplitPlan(NeuralModel* model, int* stages, int stageCapacity, unsigned short* wsplit, long long wsplitCapacity, long long* wsplitCount);
/* tests / tuning: 0 = WaveNet models with a compile-time specialised layer chain run on the stage interpreter instead (same stream state,
 * bit-identical results); process-wide, set it only while no other thread is processing */
NA_EXTERN void NA_DebugSetWaveNetSpec(int on);
/* Tests / tuning: the stream count of one recurrent launch from which the four-streams-per-wave kernel is used (0: never; default 3072,
 * environment NA_REC_QUAD_MIN); returns the previous value.  NA_DebugRecurrentQuadLaunches: launches of that kernel so far. */
NA_EXTERN int NA_DebugSetRecurrentQuadMin(int streams);
NA_EXTERN long long NA_DebugRecurrentQuadLaunches(void);
/* Tests: how the runtime-shaped recurrent kernel (RecurrentWaveRtKernel) runs a recurrent model, host side only (no device needed):
 * out = { 1 if the model runs on that kernel, waves per stream (1: wave fences; 2 .. 16: a workgroup with barriers), gate rows per lane,
 * 1 if the gate weights are streamed from L2 (0: they sit in LDS), 1 if the head is evaluated inside the sample loop, dynamic LDS bytes };
 * the launcher reads the same plan.  Returns 0, or -1 when the model is not a single LSTM / GRU / keras stack. */
NA_EXTERN int NA_DebugRecurrentPlan(NeuralModel* model, int out[6]);
/* ... and for a shape alone (cell: 0 LSTM, 1 GRU; tailLayers / tailWidth / tailHistory: the dense / conv1d chain of a keras stack, zeros for
 * the classic head), with rpl > 0 / forceL2w >= 0 in place of the tuning knobs NA_REC_RPL / NA_REC_L2W (0 / -1: the knobs).  Returns 1 if
 * the loader's shape predicate of this kernel admits the shape, 0 if not, -1 on a bad argument. */
NA_EXTERN int NA_DebugRecurrentShapePlan(int cell, int hidden, int numLayers, int tailLayers, int tailWidth, int tailHistory, int rpl, int forceL2w, int out[6]);
/* Tests: which kernel runs a recurrent model of this shape, host side only -- the decision a model group takes once and
 * NA_BatchStreamKernelName reports.  haveWT: the transposed weight image exists (every model with a recurrent layer).  knobMask: bit 0
 * NA_LSTM_NO_DPP, 1 NA_GRU_NO_DPP, 2 NA_LSTM_LANE_KERNEL, 3 NA_LSTM_NO_WAVE_RT, 4 NA_REC_NO_DPP32, 5 NA_REC_L2W, and rpl for NA_REC_RPL (0: the
 * default) -- the environment is not read; knobMask -1: the process's own tuning knobs.  Returns 0 when no kernel takes the shape, else 1
 * RecurrentDppKernel, 2 LstmWaveKernel, 3 GruWaveKernel, 4 RecurrentWaveRtKernel, 5 LstmBlockKernel, 6 LstmGenericKernel, 7 GruGenericKernel
 * (the name goes to outName[cap]); -1 on a bad argument. */
NA_EXTERN int NA_DebugRecurrentKernel(int cell, int hidden, int numLayers, int tailLayers, int tailWidth, int tailHistory, int haveWT, int knobMask, int rpl,
	char* outName, int cap);
/* Tests: the WaveNet counterparts, host side only.  Knobs of both: bit i of knobMask set = knob i takes knobs[i], every other knob its
 * default -- the environment is not read; knobMask -1: the process's own tuning knobs.  Knob order: 0 NA_WN_KERNEL (1 split, 2 frame,
 * 3 generic), 1 NA_WN_PACK, 2 NA_WN_PAD off, 3 NA_WN_DENSE, 4 NA_SP_T, 5 NA_SP_SPB, 6 NA_SP_GEN, 7 NA_SP_NO_T1, 8 NA_FR_PF, 9 NA_FR_SPB,
 * 10 specialised chains on (NA_WN_SPEC).
 * NA_DebugWaveNetKernel: what a batch's model group decides once for `streams` streams of the model at `quality`: out = { family (1
 * f16-split, 2 frame, 3 generic), pack, dense pack, packed or padded, specialised chain (0 none, 1 Standard, 2 lite 16 / 8, 3 lite 16 / 16,
 * 4 A2 Full, 5 A2 Lite), launch kind (0 frame list, 1 split list, 2 packed list, 4 a launch of its own, 5 split, joins the packed list),
 * range proven, weights ok }, the input limit, and the kernel name NA_BatchStreamKernelName would report.  0, or -1.
 * NA_DebugWaveNetLaunch: what ONE launch of n frames decides.  frame: the frame-kernel list (else a list of the f16-split kernels);
 * groupFacts: 8 ints per group = { specialised chain, pack, fewest tiles per wave of the fast interpreter (0: generic), (virtual) streams,
 * index lists present, largest staged block of the frame kernel (floats), most channel groups, most operands per stage }; sharing:
 * launches that share the chip; beyondCache: the state exceeds the Infinity Cache; cus: compute units.  out = { kernel (0 none, 1 chain,
 * 2 chain as a table launch, 3 stage interpreter, 4 frame kernel, 5 the caller cuts the list into launches of eight), hipError_t of a
 * refusal, chain family member (0 Std, 1 Lite, 2 LitePacked, 3 Lite16T1, 4 A2), NF, SPB, NT, T, WPS, GEN, PK, PF }.  0, or -1. */
NA_EXTERN int NA_DebugWaveNetKernel(NeuralModel* model, float quality, int streams, int knobMask, const int* knobs, int out[8], float* inputLimit, char* outName, int cap);
NA_EXTERN int NA_DebugWaveNetLaunch(int frame, int n, int numGroups, const int* groupFacts, int sharing, int beyondCache, int cus, int knobMask, const int* knobs,
	int out[11]);
/* Tests: export / import kernel launches of the stream snapshots so far (one per model group and call, whatever the stream count) */
NA_EXTERN long long NA_DebugSnapshotLaunches(void);
/* Tests: which implementation of the NCCL entry points the multi-GPU host binds.  0 = librccl.so (the product).  1 = a loopback table
 * inside this library (csrc/rccl_loopback.cpp): every rank may sit on the SAME device and a transfer is a device-to-device copy, so the
 * multi-rank orchestration (communicators, weight fan-out, gathered fan-in, failure teardown) executes on a one-GPU box; it moves no
 * byte over xGMI.  failSendAt > 0 makes the failSendAt-th ncclSend of the loopback table fail (fault injection), rendezvousMs > 0 is how
 * long a loopback rank waits for a peer that never posts.  Set it while no multi batch is being committed. */
NA_EXTERN void NA_DebugSetRcclApi(int mode, int failSendAt, int rendezvousMs);
/* Tests: a kernel that keeps the batch's streams busy for `milliseconds` (at most 10 000) behind whatever they hold -- a device that
 * does not answer, as far as the waits of this batch can tell (tests/test_gpu_stall.py drives the wait limit with it). */
NA_EXTERN int NA_DebugStallDevice(NA_Batch* batch, double milliseconds);
/* Tests: the route the batch's last processing call took (csrc/host_route.h HostRoute, DESIGN.md 2.4 "Routes"), -1 before any call.
 * NA_BatchProcess: 0 registered blocks in place, 1 staged in halves, 2 staged in place, 3 staged through the copy engines;
 * NA_BatchSubmit: 4 the chains, 5 in place on the batch stream, 6 the slot's own stream, 7 the copy streams;
 * NA_BatchProcessDevice: 8 resident launch, 9 the chains, 10 ordered; host rows to device rows (the multi-GPU host): 11 in place, 12 copied. */
NA_EXTERN int NA_DebugLastHostRoute(NA_Batch* batch);
/* ... and of the batch of one shard of a multi-GPU host (the only caller of the host-rows-to-device-rows entry point: RCCL fan-in) */
NA_EXTERN int NA_DebugMultiLastHostRoute(NA_MultiBatch* multi, int shard);
/* Tests: hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipStreamCreate* / hipEventCreate* calls the library has made in this process
 * so far -- a real-time safe call leaves the count where it was (tests/test_gpu_pool.py) */
NA_EXTERN long long NA_DebugDeviceResourceCalls(void);
/* Tests: the model-rate input and output rows ([streams][*frames], rows *frames floats apart) of the LAST processing call of a resampling
 * batch -- of its last piece where a call longer than 2048 external samples ran in several -- copied to the host; either pointer may be
 * NULL.  Fails if *frames exceeds capacityPerRow.  Synchronises the batch. */
NA_EXTERN int NA_DebugResampleTap(NA_Batch* batch, float* modelIn, float* modelOut, long long capacityPerRow, int* frames);
/* Tests: the NEXT NA_RenderOfflineAtRate (one call) copies job 0's model-rate input u and output v, M frames each, to these host arrays
 * (either may be NULL); that call fails before any device work if M > capacity.  Both NULL: off. */
NA_EXTERN void NA_DebugSetRenderTap(float* modelIn, float* modelOut, long long capacity);
/* tuning aid: device buffer (long long[stages*4*waves]) that workgroup 0 of the WaveNet kernel stamps with the shader clock; NULL = off */
NA_EXTERN void NA_DebugSetTraceBuffer(void* deviceBuffer);
/* Tests: runs on [NA_BatchNumStreams][n] host rows (`stride` floats apart), in place of model outputs, exactly what a processing call
 * of n samples runs for the cabinet stage: table, launches, book advance.  Synchronous; set-up side (it allocates a device block). */
NA_EXTERN int NA_DebugRunCabinetStage(NA_Batch* batch, float* hostRows, long stride, size_t n);
/* Tests: launches of the cabinet stage's kernels so far (two per piece of a call with entries) */
NA_EXTERN long long NA_DebugCabinetLaunches(void);
/* Tests: as NA_DebugRunCabinetStage, for the reverb stage: the stage alone on given rows -- table, launches, book advance */
NA_EXTERN int NA_DebugRunReverbStage(NA_Batch* batch, float* hostRows, long stride, size_t n);
/* Tests: launches of the reverb stage's processing kernels so far (per piece of a call with entries: append and apply, the spectrum
 * launch where the piece completes a block of some entry, the tail launch where some entry needs a tail) */
NA_EXTERN long long NA_DebugReverbLaunches(void);
/* Tests: copies the reverb transform's twiddle table out -- 256 floats, W[q] = (out[2q], out[2q + 1]), q in [0, 128) -- so that a
 * restatement uses the library's own values; returns 256, or -1 when `floats` < 256.  Needs no batch. */
NA_EXTERN int NA_DebugReverbTwiddles(float* out, int floats);
/* Tests: as NA_DebugRunCabinetStage, for the delay stage: the stage alone on given rows -- table, launches, book advance */
NA_EXTERN int NA_DebugRunDelayStage(NA_Batch* batch, float* hostRows, long stride, size_t n);
/* Tests: launches of the delay stage's kernel so far (one per piece of a call with entries) */
NA_EXTERN long long NA_DebugDelayLaunches(void);
/* Tests: as NA_DebugRunCabinetStage, for the compressor stage: the stage alone on given rows -- table, launch, book advance */
NA_EXTERN int NA_DebugRunCompressorStage(NA_Batch* batch, float* hostRows, long stride, size_t n);
/* Tests: launches of the compressor stage's kernel so far (one per processing call with entries) */
NA_EXTERN long long NA_DebugCompressorLaunches(void);
/* Tests: as NA_DebugRunCabinetStage, for the modulation stage: the stage alone on given rows -- table, launches, book advance */
NA_EXTERN int NA_DebugRunModStage(NA_Batch* batch, float* hostRows, long stride, size_t n);
/* Tests: launches of the modulation stage's kernel so far (one per piece of a call with entries) */
NA_EXTERN long long NA_DebugModLaunches(void);
/* Tests: launches of the gate stage's two kernels so far (two per processing call with entries) */
NA_EXTERN long long NA_DebugGateLaunches(void);
/* Tests: launches of the meter stage's two kernels so far (two per processing call with entries) */
NA_EXTERN long long NA_DebugMeterLaunches(void);
/* Tests: launches of the tuner stage's two kernels so far (one append per piece of a call with entries, one evaluate where an evaluation ends) */
NA_EXTERN long long NA_DebugTunerLaunches(void);
/* Tests: launches of the EQ stage's kernel so far (one per processing call with entries) */
NA_EXTERN long long NA_DebugEqLaunches(void);
/* Tests: as NA_DebugRunCabinetStage, for the EQ stage: the stage alone on given rows -- table, launch, book advance */
NA_EXTERN int NA_DebugRunEqStage(NA_Batch* batch, float* hostRows, long stride, size_t n);
/* Tests: launches of the mix stage's MixStageKernel so far (one per processing call with groups) and of its MixStashKernel (one per
 * processing call while some group has a DRY member) */
NA_EXTERN long long NA_DebugMixLaunches(void);
NA_EXTERN long long NA_DebugMixStashLaunches(void);
/* Tests: as NA_DebugRunCabinetStage, for the mix stage, with what the stage runs in front of the models on the input rows `hostIn`
 * (same shape as hostRows; may be NULL when no group has a DRY member): table, stash launch, mix launch, book advance */
NA_EXTERN int NA_DebugRunMixStage(NA_Batch* batch, const float* hostIn, float* hostRows, long stride, size_t n);
#endif /* NA_RELEASE */

#ifdef __cplusplus
}
#endif
#endif
