// HostPipeBench: PCIe-inclusive throughput of the batched engine from a plain C++ host, through the C ABI only
// (include/neuralaudio_amd.h): host buffers in, host buffers out, pipelined with NA_BatchSubmit / NA_BatchCollect.
//   HostPipeBench <model file> [streams=1024] [frames=128] [buffers=2000]
//   HostPipeBench <model file> [streams] [frames] [buffers] --gpus N [--devices 0,0,...] [--fan-in rccl] [--loopback]
//       the multi-GPU host (NA_Multi*: one batch + one host thread + one HIP stream per device, the global stream list sharded by
//       cost): `streams` is the GLOBAL count; --devices names the device of every shard explicitly (an index may repeat, e.g. 0,0 runs
//       two shards on one GPU -- the plumbing test on a single-GPU box).  A second model file may follow --mix: the global list is then
//       half / half (architecture-sorted), which exercises the cost-balanced cut.
//   HostPipeBench <model file> [streams] [frames] [buffers=64] --migrate K [--devices a,b]
//       the stream-snapshot example (RunMigrate below): moves K streams half way through and checks the result against an unmoved run.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --churn K [--churn-legacy] [--churn-every E=10]
//       join and leave on a batch that never stops (RunChurn below): every E-th buffer K streams leave or come back -- through the pool
//       (NA_BatchParkStream / NA_BatchActivateStream) or, with --churn-legacy, through NA_BatchRemoveStreams / NA_BatchAddStreams.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --handover K [--mix <model 2>] [--fade N=256]
//       the click-free model switch on a batch that never stops (RunHandover below): every K-th buffer one of 16 sessions is handed over
//       (NA_BatchHandover) to a parked stream of the other model (--mix), with one model to a second stream of it.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --cab TAPS [--cab-irs M=1]
//       the cabinet stage on a batch that never stops (RunCabinet below): M impulse responses of TAPS taps spread over the streams.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --gate K
//       the plain run below with the gate stage enabled and noise gates on the first K streams (K = 0: enabled, no gate set: must cost
//       nothing); adds the device span per buffer of the pipelined loop between the library's event marks.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --eq K [--eq-sections S=3]
//       the plain run below with the EQ stage enabled and an S-section cascade on the first K streams -- low shelf, peak, high shelf,
//       then further peaks up to 8 -- (K = 0: enabled, no EQ set: must cost nothing); the same device span as --gate.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --meter K [--meter-window W=1024]
//       the plain run below with the meter stage enabled and meters of W samples on the first K streams (K = 0: enabled, no meter set:
//       must cost nothing); the pipelined loop reads the first stream's meter behind every buffer (NA_BatchReadStreamMeter: no wait);
//       the same device span as --gate.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --tuner K [--tuner-hop H] [--tuner-stagger]
//       the plain run below with the tuner stage enabled and a guitar-range tuner (NA_TunerParamsFromRange: 41.2 Hz .. 1320 Hz at 48 kHz,
//       30 evaluations a second; H: hopSamples instead) on the first K streams (K = 0: enabled, no tuner set: must cost nothing).  Every
//       phase is 0 -- all K tuners evaluate in the same buffer -- or, with --tuner-stagger, stream i gets phase i * H / K.  The
//       pipelined loop reads the first stream's tuner behind every buffer (NA_BatchReadStreamTuner: no wait) and times every buffer
//       period (pipelined_period_us: the median, the 99th percentile and the longest); the same device span as --gate.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --mix N [--mix-dry]
//       (--mix followed by a NUMBER; followed by a file name it is the second model of the modes above.)  The plain run below with the
//       mix stage enabled and N mix groups of two neighbouring streams each -- streams 2g and 2g + 1, stereo: both rows are outputs, the
//       first panned -0.5 and the second +0.5 (NA_MixGainsFromPan) -- (N = 0: enabled, no group: must cost nothing).  With --mix-dry
//       each group gets the DRY tap of its first stream as a third member, at -6 dB in the centre.  Times every buffer period of the
//       pipelined loop like --tuner; the same device span as --gate.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --reverb N [--reverb-taps K=48000] [--reverb-irs M=1]
//       the plain run below with the reverb stage enabled (maxTaps = K) and a reverb on the first N streams: M synthetic IRs of K taps
//       (decaying noise), IR s % M on stream s, wet 0.3, dry 1 (N = 0: enabled, no reverb set: must cost nothing).  With N > 0 the run
//       first feeds ceil(K / 128) buffers, so that every delay line is full before anything is timed.  Times every buffer period like
//       --tuner; the same device span as --gate; reports the spectrum bytes the tail launch reads per buffer (input spectra: every
//       stream's own; IR spectra: the same amount, of which M IRs' worth is distinct).
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --delay N [--delay-samples D=18000]
//       the plain run below with the delay stage enabled (maxDelaySamples = D) and an echo on the first N streams: D samples (375 ms at
//       48 kHz by default), feedback 0.45, both filters in the loop, wet -6 dB, dry 0 dB (NA_DelayParamsFromMs) -- (N = 0: enabled, no
//       delay set: must cost nothing).  With N > 0 the run first feeds ceil(D / frames) buffers, so that every line is full.  Times every
//       buffer period like --tuner; the same device span as --gate.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --comp N [--comp-ms A=5 [--comp-release-ms R=100]]
//       the plain run below with the compressor stage enabled and a compressor on the first N streams: threshold -24 dB, ratio 4, knee
//       6 dB, makeup 3 dB, attack A ms, release R ms at 48 kHz (NA_CompressorParamsFromDb) -- (N = 0: enabled, no compressor set: must
//       cost nothing).  Times every buffer period like --tuner; the same device span as --gate.
//   HostPipeBench <model file> [streams] [frames] [buffers=2000] --mod N [--mod-base-ms B=7 --mod-depth-ms 3 --mod-rate-hz 0.8 --mod-voices 3 --mod-fb 0]
//       the plain run below with the modulation stage enabled (maxDelaySamples = 4096) and a modulation on the first N streams: voices a
//       1 / voices of a cycle apart around B ms at 48 kHz, "sine" shape, wet -3 dB, dry 0 dB (NA_ModParamsFromMs); the defaults are a
//       chorus, --mod-base-ms 1 --mod-fb 0.7 (depth then defaults to 0.9 ms, one voice) a flanger -- (N = 0: enabled, nothing set: must
//       cost nothing).  With N > 0 the run first feeds 4096 samples, so that every line is full.  Times every buffer period like --tuner;
//       the same device span as --gate.
// Prints one JSON object: microseconds per buffer for the copying entry points (caller-owned buffers) and for the zero-copy ones
// (NA_BatchNextInput / NA_BatchOutputView: the host produces into / consumes from the pinned staging buffers), two buffers in
// flight, plus the blocking NA_BatchProcess latency.  bench.py reports these as "pcie_inclusive" (never as `value`).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "neuralaudio_amd.h"

static double Now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "HostPipeBench: %s failed: %s\n", #cond, NA_GetLastError()); return 1; } } while (0)

static int RunMulti(NeuralModelLoader* loader, NeuralModel* model, const char* mixFile, const std::vector<int>& devices, int streams, int frames, int buffers, bool rcclFanIn)
{
	NA_MultiBatch* multi = NA_MultiCreate(devices.data(), (int)devices.size());
	CHECK(multi != nullptr);
	// --fan-in rccl: weights replicated and output rows gathered over RCCL (one rank per shard: distinct devices); blocking calls only
	if (rcclFanIn) CHECK(NA_MultiSetFanIn(multi, 1) == 0);
	NeuralModel* second = nullptr;
	if (mixFile)
	{
		second = NA_CreateModelFromFileUtf8(loader, mixFile, 0);
		CHECK(second != nullptr);
		CHECK(NA_MultiAddStreams(multi, model, 1.0f, streams / 2, 1) == 0);
		CHECK(NA_MultiAddStreams(multi, second, 1.0f, streams - streams / 2, 1) == streams / 2);
	}
	else CHECK(NA_MultiAddStreams(multi, model, 1.0f, streams, 1) == 0);
	CHECK(NA_MultiCommit(multi) == 0);
	const size_t count = (size_t)streams * frames;
	std::vector<float> in(count), out(count), ref(count);
	for (size_t i = 0; i < count; i++) in[i] = 0.25f * (float)((i * 2654435761u) >> 8 & 0xffff) / 65536.0f - 0.125f;
	// one single-device batch with the same global list: the sharded host must reproduce it bit for bit
	{
		NA_Batch* one = NA_BatchCreate(devices[0], nullptr);
		CHECK(one != nullptr);
		if (second)
		{
			CHECK(NA_BatchAddStreams(one, model, 1.0f, streams / 2, 1) == 0);
			CHECK(NA_BatchAddStreams(one, second, 1.0f, streams - streams / 2, 1) == streams / 2);
		}
		else CHECK(NA_BatchAddStreams(one, model, 1.0f, streams, 1) == 0);
		CHECK(NA_BatchProcess(one, in.data(), ref.data(), (size_t)frames) == 0);
		NA_BatchDestroy(one);
	}
	CHECK(NA_MultiProcess(multi, in.data(), out.data(), (size_t)frames) == 0);
	const bool identical = std::memcmp(out.data(), ref.data(), count * sizeof(float)) == 0;
	std::vector<double> lat;
	for (int i = 0; i < 200; i++)
	{
		const double t0 = Now();
		CHECK(NA_MultiProcess(multi, in.data(), out.data(), (size_t)frames) == 0);
		if (i >= 30) lat.push_back((Now() - t0) * 1e6);
	}
	std::sort(lat.begin(), lat.end());
	double usPipe = 0.0;
	if (!rcclFanIn)
	{
		int pending = NA_MultiSubmit(multi, in.data(), (size_t)frames);
		CHECK(pending >= 0);
		const double t0 = Now();
		for (int i = 0; i < buffers; i++)
		{
			const int next = NA_MultiSubmit(multi, in.data(), (size_t)frames);
			CHECK(next >= 0);
			CHECK(NA_MultiCollect(multi, pending, out.data()) == 0);
			pending = next;
		}
		CHECK(NA_MultiCollect(multi, pending, out.data()) == 0);
		usPipe = (Now() - t0) * 1e6 / buffers;
	}
	else
	{
		const double t0 = Now();
		for (int i = 0; i < buffers; i++) CHECK(NA_MultiProcess(multi, in.data(), out.data(), (size_t)frames) == 0);
		usPipe = (Now() - t0) * 1e6 / buffers; // (blocking calls back to back: the gathered path has no pipelined form)
	}
	std::printf("{\"multi_gpu_host\": true, \"shards\": [");
	for (int s = 0; s < NA_MultiNumShards(multi); s++)
	{
		int b = 0, e = 0, d = 0;
		CHECK(NA_MultiShardRange(multi, s, &b, &e, &d) == 0);
		std::printf("%s{\"device\": %d, \"begin\": %d, \"end\": %d}", s ? ", " : "", d, b, e);
	}
	std::printf("], \"fan_in\": \"%s\", \"streams\": %d, \"frames\": %d, \"buffers\": %d, \"matches_single_batch\": %s, \"us_per_buffer_pipelined\": %.3f, \"Msamples_per_s\": %.1f, "
		"\"blocking_latency_us\": {\"p50\": %.1f, \"p99\": %.1f}}\n",
		rcclFanIn ? "rccl" : "host rows", streams, frames, buffers, identical ? "true" : "false", usPipe, (double)count / usPipe, lat[lat.size() / 2], lat[(size_t)(lat.size() * 0.99)]);
	NA_MultiDestroy(multi);
	if (second) DeleteModel(second);
	return identical ? 0 : 3;
}

// --migrate K: the complete host example of the stream snapshots (include/neuralaudio_amd.h "stream snapshots").
// Half way through `buffers` buffers the first K streams are saved (NA_BatchSaveStreams), removed, added again as fresh streams
// without prewarm -- in a second batch on devices[1] when --devices a,b is given, else in the same batch -- and loaded
// (NA_BatchLoadStreams); the final buffer of every stream is then compared with a run in which nothing moved.  Also times the two
// calls (median of 12 after a warm-up call) and, for context, what a host without snapshots does to move a stream and lose its
// state: NA_BatchRemoveStreams + NA_BatchAddStreams(doPrewarm = 1) of the same count.
static double Median(std::vector<double> v)
{
	std::sort(v.begin(), v.end());
	return v.empty() ? 0.0 : v[v.size() / 2];
}

static int RunMigrate(NeuralModel* model, const std::vector<int>& devices, int streams, int frames, int buffers, int K)
{
	CHECK(K >= 1 && K <= streams && buffers >= 2);
	const int dev0 = devices.empty() ? 0 : devices[0];
	const bool second = devices.size() > 1;
	const size_t count = (size_t)streams * frames;
	auto fill = [&](std::vector<float>& in, int buffer) {
		for (size_t i = 0; i < in.size(); i++) in[i] = 0.5f * (float)((((i + (size_t)buffer * 7919u) * 2654435761u) >> 8) & 0xffff) / 65536.0f - 0.25f;
	};
	std::vector<float> in(count), refOut(count), out(count), outB((size_t)K * frames);
	// the unmigrated run
	{
		NA_Batch* ref = NA_BatchCreate(dev0, nullptr);
		CHECK(ref != nullptr);
		CHECK(NA_BatchAddStreams(ref, model, 1.0f, streams, 1) >= 0);
		for (int b = 0; b < buffers; b++)
		{
			fill(in, b);
			CHECK(NA_BatchProcess(ref, in.data(), refOut.data(), (size_t)frames) == 0);
		}
		NA_BatchDestroy(ref);
	}
	NA_Batch* a = NA_BatchCreate(dev0, nullptr);
	CHECK(a != nullptr);
	CHECK(NA_BatchAddStreams(a, model, 1.0f, streams, 1) >= 0);
	NA_Batch* b2 = second ? NA_BatchCreate(devices[1], nullptr) : a;
	CHECK(b2 != nullptr);
	for (int b = 0; b < buffers / 2; b++)
	{
		fill(in, b);
		CHECK(NA_BatchProcess(a, in.data(), out.data(), (size_t)frames) == 0);
	}
	std::vector<int> ids((size_t)K);
	for (int i = 0; i < K; i++) ids[(size_t)i] = i;
	const long long each = NA_BatchStreamSnapshotBytes(a, 0);
	CHECK(each > 0 && each == NA_ModelSnapshotBytes(model));
	std::vector<char> blob((size_t)each * K);
	size_t written = 0;
	CHECK(NA_BatchSaveStreams(a, ids.data(), K, blob.data(), blob.size(), &written) == 0 && written == blob.size());
	const std::string kernelFrom = NA_BatchStreamKernelName(a, 0);
	CHECK(NA_BatchRemoveStreams(a, 0, K) == 0);
	const int first = NA_BatchAddStreams(b2, model, 1.0f, K, 0); // fresh, no prewarm: the snapshot brings the state
	CHECK(first == 0);
	CHECK(NA_BatchLoadStreams(b2, ids.data(), K, blob.data(), blob.size()) == 0);
	const std::string kernelTo = NA_BatchStreamKernelName(b2, 0);
	for (int b = buffers / 2; b < buffers; b++)
	{
		fill(in, b);
		CHECK(NA_BatchProcess(a, in.data(), out.data(), (size_t)frames) == 0);
		if (second) CHECK(NA_BatchProcess(b2, in.data(), outB.data(), (size_t)frames) == 0); // (rows 0 .. K-1 of the input are the moved streams')
	}
	if (second) std::memcpy(out.data(), outB.data(), outB.size() * sizeof(float));
	double maxDiff = 0.0;
	for (size_t i = 0; i < count; i++) maxDiff = std::max(maxDiff, (double)std::fabs(out[i] - refOut[i]));
	const bool identical = std::memcmp(out.data(), refOut.data(), count * sizeof(float)) == 0;
	const bool ok = identical || (kernelFrom != kernelTo && maxDiff < 1e-4);

	// timings: host to host, median of 12
	std::vector<double> tSave, tLoad, tRejoin;
	for (int r = 0; r < 13; r++)
	{
		double t0 = Now();
		CHECK(NA_BatchSaveStreams(b2, ids.data(), K, blob.data(), blob.size(), &written) == 0);
		if (r) tSave.push_back((Now() - t0) * 1e3);
		t0 = Now();
		CHECK(NA_BatchLoadStreams(b2, ids.data(), K, blob.data(), blob.size()) == 0);
		if (r) tLoad.push_back((Now() - t0) * 1e3);
	}
	for (int r = 0; r < 6; r++)
	{
		const double t0 = Now();
		CHECK(NA_BatchRemoveStreams(b2, 0, K) == 0);
		CHECK(NA_BatchAddStreams(b2, model, 1.0f, K, 1) == 0);
		CHECK(NA_BatchSynchronize(b2) == 0);
		if (r) tRejoin.push_back((Now() - t0) * 1e3);
	}
	std::printf("{\"migrate\": %d, \"streams\": %d, \"frames\": %d, \"buffers\": %d, \"second_batch\": %s, \"kernel_from\": \"%s\", \"kernel_to\": \"%s\", "
		"\"snapshot_bytes_per_stream\": %lld, \"identical\": %s, \"max_abs_diff\": %.3g, \"save_ms\": %.3f, \"load_ms\": %.3f, \"remove_add_prewarm_ms\": %.3f}\n",
		K, streams, frames, buffers, second ? "true" : "false", kernelFrom.c_str(), kernelTo.c_str(), each, identical ? "true" : "false", maxDiff, Median(tSave),
		Median(tLoad), Median(tRejoin));
	if (second) NA_BatchDestroy(b2);
	NA_BatchDestroy(a);
	return ok ? 0 : 3;
}

// --churn K: `streams` streams run `buffers` buffers through the pipelined host interface (two tickets in flight); in front of every
// E-th buffer the first K streams leave, E buffers later they come back, and so on.  Pool variant: the streams come from
// NA_BatchReserveStreams and move with NA_BatchParkStream / NA_BatchActivateStream; --churn-legacy: NA_BatchRemoveStreams /
// NA_BatchAddStreams(doPrewarm = 1) (the ids are recycled).  Prints the cost of the calls (host wall time per event of K streams), the
// mean and the longest buffer period (Collect to Collect) of the run and of the same run without churn, and -- pool variant -- the mean
// period with the K streams parked (holes: index lists instead of the contiguous fast path) against all streams active.  The final
// buffer of the last stream, which never moved, must equal the run without churn bit for bit (exit code 3 otherwise).
struct ChurnRun
{
	double meanUs = 0.0, maxUs = 0.0, leaveUs = 0.0, joinUs = 0.0, leaveMaxUs = 0.0, joinMaxUs = 0.0, holesUs = 0.0, fullUs = 0.0;
	std::vector<float> lastRow;
};

static int RunChurnVariant(NeuralModel* model, int streams, int frames, int buffers, int K, int every, int variant /* 0 none, 1 pool, 2 legacy */, ChurnRun& result)
{
	NA_Batch* batch = NA_BatchCreate(0, nullptr);
	CHECK(batch != nullptr);
	if (variant == 1)
	{
		CHECK(NA_BatchReserveStreams(batch, model, streams, 1) == 0);
		for (int s = 0; s < streams; s++) CHECK(NA_BatchActivateStream(batch, s, 1.0f) == 0);
	}
	else CHECK(NA_BatchAddStreams(batch, model, 1.0f, streams, 1) == 0);
	const size_t count = (size_t)streams * frames;
	std::vector<std::vector<float>> in(8, std::vector<float>(count));
	for (size_t b = 0; b < in.size(); b++)
		for (size_t i = 0; i < count; i++) in[b][i] = 0.5f * (float)((((i + b * 7919u) * 2654435761u) >> 8) & 0xffff) / 65536.0f - 0.25f;
	std::vector<float> out(count);
	std::vector<double> tLeave, tJoin;
	bool away = false;
	auto event = [&]() -> int {
		const double t0 = Now();
		if (variant == 1)
			for (int s = 0; s < K; s++) CHECK((away ? NA_BatchActivateStream(batch, s, 1.0f) : NA_BatchParkStream(batch, s)) == 0);
		else if (away) CHECK(NA_BatchAddStreams(batch, model, 1.0f, K, 1) == 0);
		else CHECK(NA_BatchRemoveStreams(batch, 0, K) == 0);
		(away ? tJoin : tLeave).push_back((Now() - t0) * 1e6);
		away = !away;
		return 0;
	};
	auto loop = [&](int n, int firstBuffer, bool churn, double& meanUs, double& maxUs) -> int {
		int pending = NA_BatchSubmit(batch, in[(size_t)firstBuffer % in.size()].data(), (size_t)frames);
		CHECK(pending >= 0);
		double last = Now(), sum = 0.0;
		maxUs = 0.0;
		for (int i = 1; i <= n; i++)
		{
			if (churn && variant != 0 && i % every == 0 && i < n && event() != 0) return 1;
			int next = -1;
			if (i < n)
			{
				next = NA_BatchSubmit(batch, in[(size_t)(firstBuffer + i) % in.size()].data(), (size_t)frames);
				CHECK(next >= 0);
			}
			CHECK(NA_BatchCollect(batch, pending, out.data()) == 0);
			const double now = Now();
			if (i > 20) // (the first buffers: first-use set-up of the pipelined interface)
			{
				sum += (now - last) * 1e6;
				maxUs = std::max(maxUs, (now - last) * 1e6);
			}
			last = now;
			pending = next;
		}
		meanUs = sum / std::max(1, n - 20);
		return 0;
	};
	if (loop(buffers, 0, true, result.meanUs, result.maxUs) != 0) return 1;
	if (away && event() != 0) return 1; // everybody is back for the final buffer
	CHECK(NA_BatchProcess(batch, in[1].data(), out.data(), (size_t)frames) == 0);
	result.lastRow.assign(out.begin() + (long)((size_t)(streams - 1) * frames), out.end());
	if (variant == 1)
	{
		double ignored = 0.0;
		if (loop(std::max(buffers / 4, 40), 0, false, result.fullUs, ignored) != 0) return 1;
		for (int s = 0; s < K; s++) CHECK(NA_BatchParkStream(batch, s * 2 + 1) == 0); // (holes, not a prefix: RunChurn holds K to half the streams)
		if (loop(std::max(buffers / 4, 40), 0, false, result.holesUs, ignored) != 0) return 1;
	}
	result.leaveUs = Median(tLeave);
	result.joinUs = Median(tJoin);
	result.leaveMaxUs = tLeave.empty() ? 0.0 : *std::max_element(tLeave.begin(), tLeave.end());
	result.joinMaxUs = tJoin.empty() ? 0.0 : *std::max_element(tJoin.begin(), tJoin.end());
	NA_BatchDestroy(batch);
	return 0;
}

static int RunChurn(NeuralModel* model, int streams, int frames, int buffers, int K, int every, bool legacy)
{
	CHECK(K >= 1 && 2 * K <= streams && every >= 1 && buffers > 2 * every + 20);
	ChurnRun quiet, churned;
	if (RunChurnVariant(model, streams, frames, buffers, K, every, 0, quiet) != 0) return 1;
	if (RunChurnVariant(model, streams, frames, buffers, K, every, legacy ? 2 : 1, churned) != 0) return 1;
	const bool identical = quiet.lastRow.size() == churned.lastRow.size() &&
		std::memcmp(quiet.lastRow.data(), churned.lastRow.data(), quiet.lastRow.size() * sizeof(float)) == 0;
	std::printf("{\"churn\": %d, \"variant\": \"%s\", \"every\": %d, \"streams\": %d, \"frames\": %d, \"buffers\": %d, "
		"\"leave_us\": {\"p50\": %.1f, \"max\": %.1f}, \"join_us\": {\"p50\": %.1f, \"max\": %.1f}, "
		"\"buffer_period_us\": {\"mean\": %.1f, \"max\": %.1f}, \"no_churn_buffer_period_us\": {\"mean\": %.1f, \"max\": %.1f}, ",
		K, legacy ? "remove + add" : "pool", every, streams, frames, buffers, churned.leaveUs, churned.leaveMaxUs, churned.joinUs, churned.joinMaxUs,
		churned.meanUs, churned.maxUs, quiet.meanUs, quiet.maxUs);
	if (!legacy) std::printf("\"all_active_buffer_period_us\": %.1f, \"with_%d_parked_holes_buffer_period_us\": %.1f, ", churned.fullUs, K, churned.holesUs);
	std::printf("\"unchurned_stream_identical\": %s}\n", identical ? "true" : "false");
	return identical ? 0 : 3;
}

// --handover K: `streams` pooled streams run `buffers` buffers through the pipelined host interface (two tickets in flight).  Sixteen of
// them are sessions with a parked spare each -- of the --mix model, else of the same one; in front of every K-th buffer the next session
// in turn is handed over to its other stream with a fade of N samples and a level gain on the incoming one (a session whose last
// hand-over has not ended in its park yet is skipped and counted).  Prints the cost of the calls (host wall time), the mean and the
// longest buffer period (Collect to Collect) of that run and of the same run without the stage, and the mean period of steady states:
// stage enabled with no entry, 16 gain entries, a gain entry on every stream, 16 concurrent fades.  The final buffer of the last
// stream, which never took part, must equal the run without hand-overs bit for bit (exit code 3 otherwise).
struct HandoverRun
{
	double meanUs = 0.0, maxUs = 0.0, handoverUs = 0.0, handoverMaxUs = 0.0, gainUs = 0.0, gainMaxUs = 0.0;
	double idleUs = 0.0, gain16Us = 0.0, gainAllUs = 0.0, fades16Us = 0.0;
	int events = 0, skipped = 0;
	std::vector<float> lastRow;
};

static int RunHandoverVariant(NeuralModel* model, NeuralModel* other, int streams, int frames, int buffers, int K, int fade, bool stage, HandoverRun& result)
{
	const int sessions = 16;
	NA_Batch* batch = NA_BatchCreate(0, nullptr);
	CHECK(batch != nullptr);
	CHECK(NA_BatchReserveStreams(batch, model, streams, 1) == 0);
	CHECK(NA_BatchReserveStreams(batch, other, sessions, 1) == streams);
	for (int s = 0; s < streams; s++) CHECK(NA_BatchActivateStream(batch, s, 1.0f) == 0);
	if (stage) CHECK(NA_BatchEnableOutputStage(batch) == 0);
	const int rows = streams + sessions;
	const size_t count = (size_t)rows * frames;
	std::vector<std::vector<float>> in(8, std::vector<float>(count));
	for (size_t b = 0; b < in.size(); b++)
	{
		for (size_t i = 0; i < (size_t)streams * frames; i++) in[b][i] = 0.5f * (float)((((i + b * 7919u) * 2654435761u) >> 8) & 0xffff) / 65536.0f - 0.25f;
		// (both streams of a session take the same input: the host contract of a hand-over)
		for (int j = 0; j < sessions; j++) std::memcpy(&in[b][(size_t)(streams + j) * frames], &in[b][(size_t)j * frames], (size_t)frames * sizeof(float));
	}
	std::vector<float> out(count);
	std::vector<double> tHandover, tGain;
	const float level = (float)std::pow(10.0, (GetRecommendedOutputDBAdjustment(other) - GetRecommendedOutputDBAdjustment(model)) / 20.0);
	std::vector<char> onSpare((size_t)sessions, 0);
	int turn = 0;
	auto event = [&]() -> int {
		const int j = turn++ % sessions;
		const int from = onSpare[(size_t)j] ? streams + j : j, to = onSpare[(size_t)j] ? j : streams + j;
		if (NA_BatchHandoverRemaining(batch, from) != 0 || !NA_BatchIsParked(batch, to)) { result.skipped++; return 0; }
		double t0 = Now();
		CHECK(NA_BatchHandover(batch, from, to, 1.0f, fade) == 0);
		tHandover.push_back((Now() - t0) * 1e6);
		t0 = Now();
		CHECK(NA_BatchSetStreamGain(batch, to, onSpare[(size_t)j] ? 1.0f : level, 0) == 0);
		tGain.push_back((Now() - t0) * 1e6);
		onSpare[(size_t)j] = !onSpare[(size_t)j];
		result.events++;
		return 0;
	};
	auto loop = [&](int n, bool handovers, double& meanUs, double& maxUs) -> int {
		int pending = NA_BatchSubmit(batch, in[0].data(), (size_t)frames);
		CHECK(pending >= 0);
		double last = Now(), sum = 0.0;
		maxUs = 0.0;
		for (int i = 1; i <= n; i++)
		{
			if (handovers && stage && i % K == 0 && i < n && event() != 0) return 1;
			int next = -1;
			if (i < n)
			{
				next = NA_BatchSubmit(batch, in[(size_t)i % in.size()].data(), (size_t)frames);
				CHECK(next >= 0);
			}
			CHECK(NA_BatchCollect(batch, pending, out.data()) == 0);
			const double now = Now();
			if (i > 20) // (the first buffers: first-use set-up of the pipelined interface, the change of steady state)
			{
				sum += (now - last) * 1e6;
				maxUs = std::max(maxUs, (now - last) * 1e6);
			}
			last = now;
			pending = next;
		}
		meanUs = sum / std::max(1, n - 20);
		return 0;
	};
	if (loop(buffers, true, result.meanUs, result.maxUs) != 0) return 1;
	CHECK(NA_BatchProcess(batch, in[1].data(), out.data(), (size_t)frames) == 0);
	result.lastRow.assign(out.begin() + (long)((size_t)(streams - 1) * frames), out.begin() + (long)((size_t)streams * frames));
	if (stage)
	{
		// steady states.  First everything back to "no entry": the fades run out, every session's live stream at gain 1
		const int quiet = std::max(buffers / 4, 60), settle = fade / frames + 3;
		double ignored = 0.0;
		if (loop(settle + 21, false, ignored, ignored) != 0) return 1;
		for (int s = 0; s < rows; s++)
			if (NA_BatchIsLive(batch, s)) CHECK(NA_BatchSetStreamGain(batch, s, 1.0f, 0) == 0);
		if (loop(quiet, false, result.idleUs, ignored) != 0) return 1;
		for (int s = 0; s < sessions; s++) CHECK(NA_BatchSetStreamGain(batch, streams - 1 - s, 0.5f, 0) == 0);
		if (loop(quiet, false, result.gain16Us, ignored) != 0) return 1;
		for (int s = 0; s < rows; s++)
			if (NA_BatchIsLive(batch, s)) CHECK(NA_BatchSetStreamGain(batch, s, 0.5f, 0) == 0);
		if (loop(quiet, false, result.gainAllUs, ignored) != 0) return 1;
		for (int s = 0; s < rows; s++)
			if (NA_BatchIsLive(batch, s)) CHECK(NA_BatchSetStreamGain(batch, s, 1.0f, 0) == 0);
		for (int j = 0; j < sessions; j++)
		{
			const int from = onSpare[(size_t)j] ? streams + j : j, to = onSpare[(size_t)j] ? j : streams + j;
			CHECK(NA_BatchHandover(batch, from, to, 1.0f, 1 << 20) == 0); // (longer than the measurement: sixteen fades throughout)
		}
		if (loop(quiet, false, result.fades16Us, ignored) != 0) return 1;
	}
	result.handoverUs = Median(tHandover);
	result.gainUs = Median(tGain);
	result.handoverMaxUs = tHandover.empty() ? 0.0 : *std::max_element(tHandover.begin(), tHandover.end());
	result.gainMaxUs = tGain.empty() ? 0.0 : *std::max_element(tGain.begin(), tGain.end());
	NA_BatchDestroy(batch);
	return 0;
}

static int RunHandover(NeuralModel* model, NeuralModel* other, int streams, int frames, int buffers, int K, int fade)
{
	CHECK(K >= 1 && streams >= 33 && fade >= 0 && fade <= (1 << 20) && buffers > 60);
	HandoverRun quiet, moved;
	if (RunHandoverVariant(model, other, streams, frames, buffers, K, fade, false, quiet) != 0) return 1;
	if (RunHandoverVariant(model, other, streams, frames, buffers, K, fade, true, moved) != 0) return 1;
	const bool identical = quiet.lastRow.size() == moved.lastRow.size() &&
		std::memcmp(quiet.lastRow.data(), moved.lastRow.data(), quiet.lastRow.size() * sizeof(float)) == 0;
	std::printf("{\"handover\": %d, \"fade\": %d, \"mixed\": %s, \"streams\": %d, \"frames\": %d, \"buffers\": %d, \"events\": %d, \"skipped\": %d, "
		"\"handover_call_us\": {\"p50\": %.1f, \"max\": %.1f}, \"set_gain_call_us\": {\"p50\": %.1f, \"max\": %.1f}, "
		"\"buffer_period_us\": {\"mean\": %.1f, \"max\": %.1f}, \"no_stage_buffer_period_us\": {\"mean\": %.1f, \"max\": %.1f}, "
		"\"steady_buffer_period_us\": {\"no_entry\": %.1f, \"gain_entries_16\": %.1f, \"gain_entries_all\": %.1f, \"fades_16\": %.1f}, "
		"\"untouched_stream_identical\": %s}\n",
		K, fade, other != model ? "true" : "false", streams, frames, buffers, moved.events, moved.skipped, moved.handoverUs, moved.handoverMaxUs, moved.gainUs,
		moved.gainMaxUs, moved.meanUs, moved.maxUs, quiet.meanUs, quiet.maxUs, moved.idleUs, moved.gain16Us, moved.gainAllUs, moved.fades16Us,
		identical ? "true" : "false");
	return identical ? 0 : 3;
}

// --cab TAPS [--cab-irs M]: `streams` streams run through the pipelined host interface (two tickets in flight) in three phases of
// `buffers`, `buffers` and buffers / 4 buffers: (1) the stage enabled and no IR; (2) M synthetic IRs of TAPS taps (decaying noise) spread
// over all streams but the last, IR s % M on stream s; (3) all dry again but sixteen streams, each in a fade between two IRs that outlasts
// the phase.  Prints the mean buffer period (Collect to Collect) of every phase beside the same phases of a batch without the stage, and
// the cost of the set calls (host wall time).  The final buffer of the last stream, which stayed dry throughout, must equal the run
// without the stage bit for bit (exit code 3 otherwise).
struct CabinetRun
{
	double phaseUs[3] = { 0.0, 0.0, 0.0 }, phaseMaxUs[3] = { 0.0, 0.0, 0.0 }, setUs = 0.0, setMaxUs = 0.0, loadMs = 0.0;
	long long deviceBytes = 0;
	std::vector<float> lastRow;
};

static int RunCabinetVariant(NeuralModel* model, int streams, int frames, int buffers, int taps, int M, bool stage, CabinetRun& result)
{
	NA_Batch* batch = NA_BatchCreate(0, nullptr);
	CHECK(batch != nullptr);
	CHECK(NA_BatchAddStreams(batch, model, 1.0f, streams, 1) == 0);
	const size_t count = (size_t)streams * frames;
	std::vector<std::vector<float>> in(8, std::vector<float>(count));
	for (size_t b = 0; b < in.size(); b++)
		for (size_t i = 0; i < count; i++) in[b][i] = 0.5f * (float)((((i + b * 7919u) * 2654435761u) >> 8) & 0xffff) / 65536.0f - 0.25f;
	std::vector<float> out(count);
	std::vector<int> irs;
	std::vector<double> tSet;
	if (stage)
	{
		CHECK(NA_BatchEnableCabinetStage(batch, taps) == 0);
		const double t0 = Now();
		std::vector<float> h((size_t)taps);
		for (int m = 0; m < M; m++)
		{
			unsigned seed = 12345u + 977u * (unsigned)m;
			for (int k = 0; k < taps; k++)
			{
				seed = seed * 1664525u + 1013904223u;
				h[(size_t)k] = ((float)(seed >> 8 & 0xffff) / 32768.0f - 1.0f) * std::exp(-6.0f * (float)k / (float)taps) * 0.1f;
			}
			const int id = NA_BatchLoadIR(batch, h.data(), taps);
			CHECK(id >= 0);
			irs.push_back(id);
		}
		result.loadMs = (Now() - t0) * 1e3;
		NA_CabinetInfo info;
		CHECK(NA_BatchGetCabinetInfo(batch, &info) == 0);
		result.deviceBytes = info.deviceBytes;
	}
	auto setIR = [&](int s, int ir, int fade) -> int {
		const double t0 = Now();
		CHECK(NA_BatchSetStreamIR(batch, s, ir, fade) == 0);
		tSet.push_back((Now() - t0) * 1e6);
		return 0;
	};
	auto loop = [&](int n, double& meanUs, double& maxUs) -> int {
		int pending = NA_BatchSubmit(batch, in[0].data(), (size_t)frames);
		CHECK(pending >= 0);
		double last = Now(), sum = 0.0;
		maxUs = 0.0;
		for (int i = 1; i <= n; i++)
		{
			int next = -1;
			if (i < n)
			{
				next = NA_BatchSubmit(batch, in[(size_t)i % in.size()].data(), (size_t)frames);
				CHECK(next >= 0);
			}
			CHECK(NA_BatchCollect(batch, pending, out.data()) == 0);
			const double now = Now();
			if (i > 20) // (the first buffers: first-use set-up of the pipelined interface, the change of steady state)
			{
				sum += (now - last) * 1e6;
				maxUs = std::max(maxUs, (now - last) * 1e6);
			}
			last = now;
			pending = next;
		}
		meanUs = sum / std::max(1, n - 20);
		return 0;
	};
	if (loop(buffers, result.phaseUs[0], result.phaseMaxUs[0]) != 0) return 1;
	if (stage)
		for (int s = 0; s < streams - 1; s++)
			if (setIR(s, irs[(size_t)(s % M)], 0) != 0) return 1;
	if (loop(buffers, result.phaseUs[1], result.phaseMaxUs[1]) != 0) return 1;
	if (stage)
	{
		for (int s = 0; s < streams - 1; s++)
			if (setIR(s, s < 16 ? irs[(size_t)(s % M)] : -1, 0) != 0) return 1;
		for (int s = 0; s < 16; s++)
			if (setIR(s, irs[(size_t)((s + 1) % M)], 1 << 20) != 0) return 1; // (longer than the phase: sixteen fades throughout)
	}
	if (loop(std::max(buffers / 4, 60), result.phaseUs[2], result.phaseMaxUs[2]) != 0) return 1;
	CHECK(NA_BatchProcess(batch, in[1].data(), out.data(), (size_t)frames) == 0);
	result.lastRow.assign(out.begin() + (long)((size_t)(streams - 1) * frames), out.end());
	result.setUs = Median(tSet);
	result.setMaxUs = tSet.empty() ? 0.0 : *std::max_element(tSet.begin(), tSet.end());
	NA_BatchDestroy(batch);
	return 0;
}

static int RunCabinet(NeuralModel* model, int streams, int frames, int buffers, int taps, int M)
{
	CHECK(taps >= 1 && taps <= 8192 && M >= 1 && streams >= 18 && buffers > 60);
	CabinetRun plain, cab;
	if (RunCabinetVariant(model, streams, frames, buffers, taps, M, false, plain) != 0) return 1;
	if (RunCabinetVariant(model, streams, frames, buffers, taps, M, true, cab) != 0) return 1;
	const bool identical = plain.lastRow.size() == cab.lastRow.size() && std::memcmp(plain.lastRow.data(), cab.lastRow.data(), plain.lastRow.size() * sizeof(float)) == 0;
	const double gmac = (double)(streams - 1) * frames * taps * 1e-9;
	std::printf("{\"cab\": %d, \"irs\": %d, \"streams\": %d, \"frames\": %d, \"buffers\": %d, \"stage_device_bytes\": %lld, \"load_irs_ms\": %.3f, "
		"\"set_ir_call_us\": {\"p50\": %.2f, \"max\": %.1f}, "
		"\"buffer_period_us\": {\"no_ir\": %.1f, \"irs_on\": %.1f, \"fades_16\": %.1f, \"irs_on_max\": %.1f}, "
		"\"no_stage_buffer_period_us\": {\"phase_1\": %.1f, \"phase_2\": %.1f, \"phase_3\": %.1f}, \"irs_on_gmac_per_buffer\": %.4f, "
		"\"dry_stream_identical\": %s}\n",
		taps, M, streams, frames, buffers, cab.deviceBytes, cab.loadMs, cab.setUs, cab.setMaxUs, cab.phaseUs[0], cab.phaseUs[1], cab.phaseUs[2], cab.phaseMaxUs[1],
		plain.phaseUs[0], plain.phaseUs[1], plain.phaseUs[2], gmac, identical ? "true" : "false");
	return identical ? 0 : 3;
}

int main(int argc, char** argv)
{
	if (argc < 2) { std::fprintf(stderr, "usage: HostPipeBench <model> [streams] [frames] [buffers] [--gpus N] [--devices a,b,...] [--mix <model 2>] [--fan-in rccl] [--loopback] [--migrate K] [--churn K [--churn-legacy] [--churn-every E]] [--handover K [--fade N]] [--cab TAPS [--cab-irs M]] [--gate K] [--eq K [--eq-sections S]] [--meter K [--meter-window W]] [--tuner K [--tuner-hop H] [--tuner-stagger]] [--mix N [--mix-dry]] [--reverb N [--reverb-taps K] [--reverb-irs M]] [--delay N [--delay-samples D]] [--comp N [--comp-ms A] [--comp-release-ms R]] [--mod N [--mod-base-ms B] [--mod-depth-ms D] [--mod-rate-hz R] [--mod-voices V] [--mod-fb F]]\n"); return 2; }
	std::vector<const char*> pos;
	std::vector<int> devices;
	int gpus = 0;
	const char* mixFile = nullptr;
	bool rcclFanIn = false;
	int migrate = 0, churn = 0, churnEvery = 10, handover = 0, fade = 256, cab = 0, cabIRs = 1, gate = -1, eq = -1, eqSections = 3, meter = -1, meterWindow = 1024, tuner = -1, tunerHop = 0;
	int mixGroups = -1, reverb = -1, reverbTaps = 48000, reverbIRs = 1, delay = -1, delaySamples = 18000;
	int comp = -1;
	int mod = -1, modVoices = -1;
	double modBaseMs = 7.0, modDepthMs = -1.0, modRateHz = 0.8, modFb = 0.0;
	float compAttackMs = 5.0f, compReleaseMs = 100.0f;
	bool churnLegacy = false, tunerStagger = false, mixDry = false;
	for (int i = 1; i < argc; i++)
	{
		if (!std::strcmp(argv[i], "--gpus") && i + 1 < argc) gpus = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--fan-in") && i + 1 < argc) rcclFanIn = !std::strcmp(argv[++i], "rccl");
		else if (!std::strcmp(argv[i], "--mix") && i + 1 < argc)
		{
			// a number: that many mix groups (the mix stage); anything else: the second model's file
			const char* arg = argv[++i];
			if (*arg && std::strspn(arg, "0123456789") == std::strlen(arg)) mixGroups = std::atoi(arg);
			else mixFile = arg;
		}
		else if (!std::strcmp(argv[i], "--mix-dry")) mixDry = true;
		else if (!std::strcmp(argv[i], "--migrate") && i + 1 < argc) migrate = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--churn") && i + 1 < argc) churn = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--churn-every") && i + 1 < argc) churnEvery = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--churn-legacy")) churnLegacy = true;
		else if (!std::strcmp(argv[i], "--handover") && i + 1 < argc) handover = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--fade") && i + 1 < argc) fade = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--cab") && i + 1 < argc) cab = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--cab-irs") && i + 1 < argc) cabIRs = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--reverb") && i + 1 < argc) reverb = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--reverb-taps") && i + 1 < argc) reverbTaps = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--reverb-irs") && i + 1 < argc) reverbIRs = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--delay") && i + 1 < argc) delay = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--delay-samples") && i + 1 < argc) delaySamples = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--comp") && i + 1 < argc) comp = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--mod") && i + 1 < argc) mod = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--mod-base-ms") && i + 1 < argc) modBaseMs = std::atof(argv[++i]);
		else if (!std::strcmp(argv[i], "--mod-depth-ms") && i + 1 < argc) modDepthMs = std::atof(argv[++i]);
		else if (!std::strcmp(argv[i], "--mod-rate-hz") && i + 1 < argc) modRateHz = std::atof(argv[++i]);
		else if (!std::strcmp(argv[i], "--mod-voices") && i + 1 < argc) modVoices = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--mod-fb") && i + 1 < argc) modFb = std::atof(argv[++i]);
		else if (!std::strcmp(argv[i], "--comp-ms") && i + 1 < argc) compAttackMs = (float)std::atof(argv[++i]);
		else if (!std::strcmp(argv[i], "--comp-release-ms") && i + 1 < argc) compReleaseMs = (float)std::atof(argv[++i]);
		else if (!std::strcmp(argv[i], "--gate") && i + 1 < argc) gate = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--eq") && i + 1 < argc) eq = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--meter") && i + 1 < argc) meter = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--meter-window") && i + 1 < argc) meterWindow = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--tuner") && i + 1 < argc) tuner = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--tuner-hop") && i + 1 < argc) tunerHop = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--tuner-stagger")) tunerStagger = true;
		else if (!std::strcmp(argv[i], "--eq-sections") && i + 1 < argc) eqSections = std::atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "--loopback"))
		{
			// rehearsal on a one-GPU box: the multi-GPU host bound to the library's loopback RCCL table (test build only), so that
			// `--devices 0,0 --fan-in rccl` runs the communicator set-up, the weight fan-out and the gathered fan-in with two ranks
			NA_DebugSetRcclApi(1, 0, 0);
		}
		else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc)
		{
			for (const char* p = argv[++i]; *p;)
			{
				devices.push_back(std::atoi(p));
				while (*p && *p != ',') p++;
				if (*p == ',') p++;
			}
		}
		else pos.push_back(argv[i]);
	}
	const int streams = pos.size() > 1 ? std::atoi(pos[1]) : 1024, frames = pos.size() > 2 ? std::atoi(pos[2]) : 128, buffers = pos.size() > 3 ? std::atoi(pos[3]) : 2000;
	NeuralModelLoader* loader = CreateLoader();
	CHECK(loader != nullptr);
	NeuralModel* model = NA_CreateModelFromFileUtf8(loader, pos[0], 0);
	CHECK(model != nullptr);
	if (migrate > 0)
	{
		const int rc = RunMigrate(model, devices, streams, frames, pos.size() > 3 ? buffers : 64, migrate);
		DeleteModel(model);
		DeleteLoader(loader);
		return rc;
	}
	if (churn > 0)
	{
		const int rc = RunChurn(model, streams, frames, buffers, churn, churnEvery, churnLegacy);
		DeleteModel(model);
		DeleteLoader(loader);
		return rc;
	}
	if (cab > 0)
	{
		const int rc = RunCabinet(model, streams, frames, buffers, cab, cabIRs);
		DeleteModel(model);
		DeleteLoader(loader);
		return rc;
	}
	if (handover > 0)
	{
		NeuralModel* second = mixFile ? NA_CreateModelFromFileUtf8(loader, mixFile, 0) : nullptr;
		CHECK(!mixFile || second != nullptr);
		const int rc = RunHandover(model, second ? second : model, streams, frames, buffers, handover, fade);
		if (second) DeleteModel(second);
		DeleteModel(model);
		DeleteLoader(loader);
		return rc;
	}
	if (gpus > 0 || !devices.empty())
	{
		if (devices.empty())
			for (int d = 0; d < gpus; d++) devices.push_back(d);
		const int rc = RunMulti(loader, model, mixFile, devices, streams, frames, buffers, rcclFanIn);
		DeleteModel(model);
		DeleteLoader(loader);
		return rc;
	}
	NA_Batch* batch = NA_BatchCreate(0, nullptr);
	CHECK(batch != nullptr);
	CHECK(NA_BatchAddStreams(batch, model, 1.0f, streams, 1) >= 0);
	if (gate >= 0)
	{
		// thresholds around the input's level (+-0.125, a power of ~5e-3), so that the gates open and close on the signal itself
		CHECK(NA_BatchEnableGateStage(batch) == 0);
		NA_GateParams gp;
		CHECK(NA_GateParamsFromDb(48000, -20.0f, -26.0f, -60.0f, 1.0f, 1.0f, 5.0f, 20.0f, &gp) == 0);
		for (int s = 0; s < std::min(gate, streams); s++) CHECK(NA_BatchSetStreamGate(batch, s, &gp, 1) == 0);
	}
	if (comp >= 0)
	{
		// a threshold below the models' output level, so that the follower moves the gain on the signal itself
		CHECK(NA_BatchEnableCompressorStage(batch) == 0);
		static NA_CompressorParams cp;
		CHECK(NA_CompressorParamsFromDb(48000, -24.0f, 4.0f, 6.0f, 3.0f, compAttackMs, compReleaseMs, &cp) == 0);
		for (int s = 0; s < std::min(comp, streams); s++) CHECK(NA_BatchSetStreamCompressor(batch, s, &cp, 0) == 0);
	}
	if (eq >= 0)
	{
		// a tone stack: low shelf, mid peak, high shelf; more sections are further peaks
		CHECK(NA_BatchEnableEqStage(batch) == 0);
		CHECK(eqSections >= 1 && eqSections <= NA_EQ_MAX_SECTIONS);
		NA_EqSection sec[NA_EQ_MAX_SECTIONS];
		for (int i = 0; i < eqSections; i++)
		{
			const int kind = i == 0 ? 2 : (i == 2 ? 3 : 4);
			const double freq = i == 0 ? 120.0 : (i == 2 ? 6000.0 : 400.0 * (1 + i));
			CHECK(NA_EqSectionFromDesign(kind, 48000.0, freq, 0.8, i % 2 ? -4.0 : 5.0, &sec[i]) == 0);
		}
		for (int s = 0; s < std::min(eq, streams); s++) CHECK(NA_BatchSetStreamEq(batch, s, sec, eqSections, 0) == 0);
	}
	if (meter >= 0)
	{
		// a clip light at the input's peak level (+-0.125) and an output clip level of 1
		CHECK(NA_BatchEnableMeterStage(batch) == 0);
		NA_MeterParams mp = { meterWindow, 0.12f, 1.0f };
		for (int s = 0; s < std::min(meter, streams); s++) CHECK(NA_BatchSetStreamMeter(batch, s, &mp) == 0);
	}
	if (tuner >= 0)
	{
		CHECK(NA_BatchEnableTunerStage(batch) == 0);
		NA_TunerParams tp;
		CHECK(NA_TunerParamsFromRange(48000.0, 41.2, 1320.0, 30.0, &tp) == 0);
		if (tunerHop > 0) tp.hopSamples = tunerHop;
		tunerHop = tp.hopSamples;
		const int tuned = std::min(tuner, streams);
		for (int s = 0; s < tuned; s++)
		{
			tp.phase = tunerStagger ? (int)((long long)s * tp.hopSamples / tuned) : 0;
			CHECK(NA_BatchSetStreamTuner(batch, s, &tp) == 0);
		}
	}
	if (mixGroups >= 0)
	{
		CHECK(NA_BatchEnableMixStage(batch) == 0);
		mixGroups = std::min(mixGroups, streams / 2);
		float l0, r0, l1, r1, lc, rc;
		CHECK(NA_MixGainsFromPan(0.0, -0.5, &l0, &r0) == 0 && NA_MixGainsFromPan(0.0, 0.5, &l1, &r1) == 0 && NA_MixGainsFromPan(-6.0, 0.0, &lc, &rc) == 0);
		for (int g = 0; g < mixGroups; g++)
		{
			const int ids[3] = { 2 * g, 2 * g + 1, 2 * g };
			const int taps[3] = { NA_MIX_TAP_OUT, NA_MIX_TAP_OUT, NA_MIX_TAP_DRY };
			const float stereo[4] = { l0, l1, r0, r1 }, withDry[6] = { l0, l1, lc, r0, r1, rc };
			CHECK(NA_BatchSetMixGroup(batch, ids, taps, mixDry ? 3 : 2, 2, mixDry ? withDry : stereo, 0) == 0);
		}
	}
	long long reverbBytes = 0, reverbInputSpectrumBytes = 0, reverbDistinctIRBytes = 0;
	double reverbLoadMs = 0.0;
	if (reverb >= 0)
	{
		CHECK(reverbTaps >= 1 && reverbIRs >= 1);
		CHECK(NA_BatchEnableReverbStage(batch, reverbTaps) == 0);
		reverb = std::min(reverb, streams);
		reverbIRs = std::min(reverbIRs, std::max(reverb, 1));
		std::vector<int> ids;
		std::vector<float> h((size_t)reverbTaps);
		const double t0 = Now();
		for (int m = 0; m < reverbIRs && reverb > 0; m++)
		{
			unsigned seed = 12345u + 977u * (unsigned)m;
			for (int k = 0; k < reverbTaps; k++)
			{
				seed = seed * 1664525u + 1013904223u;
				h[(size_t)k] = ((float)(seed >> 8 & 0xffff) / 32768.0f - 1.0f) * std::exp(-6.0f * (float)k / (float)reverbTaps) * 0.02f;
			}
			const int id = NA_BatchLoadReverbIR(batch, h.data(), reverbTaps);
			CHECK(id >= 0);
			ids.push_back(id);
		}
		reverbLoadMs = (Now() - t0) * 1e3;
		for (int s = 0; s < reverb; s++) CHECK(NA_BatchSetStreamReverb(batch, s, ids[(size_t)(s % reverbIRs)], 0.3f, 1.0f, 0) == 0);
		NA_ReverbInfo info;
		CHECK(NA_BatchGetReverbInfo(batch, &info) == 0);
		reverbBytes = info.deviceBytes;
		const long long tailPartitions = (reverbTaps + info.partitionSamples - 1) / info.partitionSamples - 1;
		reverbInputSpectrumBytes = (long long)reverb * tailPartitions * 2048 * ((frames + info.partitionSamples - 1) / info.partitionSamples);
		reverbDistinctIRBytes = reverb > 0 ? (long long)reverbIRs * tailPartitions * 2048 : 0;
	}
	long long modBytes = 0;
	if (mod >= 0)
	{
		// a chorus by default; with feedback a flanger: one voice, a sweep just below the base
		if (modVoices < 0) modVoices = modFb != 0.0 ? 1 : 3;
		if (modDepthMs < 0.0) modDepthMs = modFb != 0.0 ? 0.9 * modBaseMs : 3.0;
		CHECK(NA_BatchEnableModStage(batch, 4096) == 0);
		mod = std::min(mod, streams);
		NA_ModParams mp;
		CHECK(NA_ModParamsFromMs(48000, modBaseMs, modDepthMs, modRateHz, NA_MOD_SINE, modVoices, modFb, -3.0, 0.0, 0.0, &mp) == 0);
		for (int s = 0; s < mod; s++) CHECK(NA_BatchSetStreamMod(batch, s, &mp, 0) == 0);
		NA_ModInfo info;
		CHECK(NA_BatchGetModInfo(batch, &info) == 0);
		modBytes = info.deviceBytes;
	}
	long long delayBytes = 0;
	if (delay >= 0)
	{
		CHECK(delaySamples >= 1);
		CHECK(NA_BatchEnableDelayStage(batch, delaySamples) == 0);
		delay = std::min(delay, streams);
		NA_DelayParams echo;
		CHECK(NA_DelayParamsFromMs(48000, 375.0, 0.45, 120.0, 4500.0, -6.0, 0.0, &echo) == 0);
		echo.delaySamples = delaySamples;
		for (int s = 0; s < delay; s++) CHECK(NA_BatchSetStreamDelay(batch, s, &echo, 0) == 0);
		NA_DelayInfo info;
		CHECK(NA_BatchGetDelayInfo(batch, &info) == 0);
		delayBytes = info.deviceBytes;
	}
	unsigned long long meterWindows = 0; // (--meter: `windows` of the last reading of stream 0 in the pipelined loop)
	unsigned long long tunerEvaluations = 0; // (--tuner: `evaluations` of the last reading of stream 0 in the pipelined loop)
	std::vector<double> periods;             // (--tuner, --mix N: every buffer period of the pipelined loop)
	const bool marks = gate >= 0 || comp >= 0 || mod >= 0 || eq >= 0 || meter >= 0 || tuner >= 0 || mixGroups >= 0 || reverb >= 0 || delay >= 0; // (the plain run stays what it was)
	const size_t count = (size_t)streams * frames;
	std::vector<float> in(count), out(count);
	for (size_t i = 0; i < count; i++) in[i] = 0.25f * (float)((i * 2654435761u) >> 8 & 0xffff) / 65536.0f - 0.125f;

	// (--reverb N > 0: the delay lines fill first -- the tail of a block sums over as many partitions as the history has)
	if (reverb > 0)
		for (long long fed = 0; fed < reverbTaps; fed += frames) CHECK(NA_BatchProcess(batch, in.data(), out.data(), (size_t)frames) == 0);

	// (--delay N > 0: the lines fill first -- from then on every read of a ring is a read of a sample the stage wrote)
	if (mod > 0)
		for (long long fed = 0; fed < 4096; fed += frames) CHECK(NA_BatchProcess(batch, in.data(), out.data(), (size_t)frames) == 0);
	if (delay > 0)
		for (long long fed = 0; fed < delaySamples; fed += frames) CHECK(NA_BatchProcess(batch, in.data(), out.data(), (size_t)frames) == 0);

	// blocking call, one buffer at a time
	std::vector<double> lat;
	for (int i = 0; i < 300; i++)
	{
		const double t0 = Now();
		CHECK(NA_BatchProcess(batch, in.data(), out.data(), (size_t)frames) == 0);
		if (i >= 50) lat.push_back((Now() - t0) * 1e6);
	}
	std::sort(lat.begin(), lat.end());

	// blocking call on blocks the host registered once (NA_RegisterHostBuffer): the kernels run on the caller's memory, no staging copies
	std::vector<double> latReg;
	{
		std::vector<float> rin(in), rout(count);
		CHECK(NA_RegisterHostBuffer(rin.data(), count * sizeof(float)) == 0);
		CHECK(NA_RegisterHostBuffer(rout.data(), count * sizeof(float)) == 0);
		for (int i = 0; i < 300; i++)
		{
			const double t0 = Now();
			CHECK(NA_BatchProcess(batch, rin.data(), rout.data(), (size_t)frames) == 0);
			if (i >= 50) latReg.push_back((Now() - t0) * 1e6);
		}
		CHECK(NA_UnregisterHostBuffer(rin.data()) == 0);
		CHECK(NA_UnregisterHostBuffer(rout.data()) == 0);
		std::sort(latReg.begin(), latReg.end());
	}

	// the same blocking step through the in-place entry points: the producer writes the pinned input slot, the consumer reads the pinned
	// output slot (no host-side copy of the two 512 KB blocks); latency = Submit .. Collect
	std::vector<double> latInPlace;
	for (int i = 0; i < 300; i++)
	{
		float* slot = NA_BatchNextInput(batch, (size_t)frames);
		CHECK(slot != nullptr);
		std::memcpy(slot, in.data(), count * sizeof(float)); // the producer's write (not part of the latency: a producer writes its samples here anyway)
		const double t0 = Now();
		const int t = NA_BatchSubmit(batch, nullptr, (size_t)frames);
		CHECK(t >= 0);
		CHECK(NA_BatchCollect(batch, t, nullptr) == 0);
		if (i >= 50) latInPlace.push_back((Now() - t0) * 1e6);
	}
	std::sort(latInPlace.begin(), latInPlace.end());

	// copying entry points, two buffers in flight (between the library's event marks: the device's span of the same loop)
	int pending = NA_BatchSubmit(batch, in.data(), (size_t)frames);
	CHECK(pending >= 0);
	if (marks) CHECK(NA_BatchMarkTime(batch, 0) == 0);
	double t0 = Now();
	for (int i = 0; i < buffers; i++)
	{
		const int next = NA_BatchSubmit(batch, in.data(), (size_t)frames);
		CHECK(next >= 0);
		CHECK(NA_BatchCollect(batch, pending, out.data()) == 0);
		pending = next;
		if (meter > 0)
		{
			NA_MeterReading reading;
			const int have = NA_BatchReadStreamMeter(batch, 0, &reading);
			CHECK(have >= 0);
			if (have) meterWindows = reading.windows;
		}
		if (tuner > 0)
		{
			NA_TunerReading reading;
			const int have = NA_BatchReadStreamTuner(batch, 0, &reading);
			CHECK(have >= 0);
			if (have) tunerEvaluations = reading.evaluations;
		}
		if (tuner >= 0 || mixGroups >= 0 || reverb >= 0 || delay >= 0 || comp >= 0 || mod >= 0) periods.push_back(Now());
	}
	CHECK(NA_BatchCollect(batch, pending, out.data()) == 0);
	const double usCopy = (Now() - t0) * 1e6 / buffers;
	double periodP50 = 0.0, periodP99 = 0.0, periodMax = 0.0;
	if (periods.size() > 1)
	{
		for (size_t i = periods.size() - 1; i > 0; i--) periods[i] = (periods[i] - periods[i - 1]) * 1e6;
		periods.erase(periods.begin());
		std::sort(periods.begin(), periods.end());
		periodP50 = periods[periods.size() / 2];
		periodP99 = periods[(size_t)(periods.size() * 0.99)];
		periodMax = periods.back();
	}
	double usMarked = 0.0; // (--gate / --eq / --meter / --tuner / --mix N only)
	if (marks)
	{
		CHECK(NA_BatchMarkTime(batch, 1) == 0);
		usMarked = (double)NA_BatchElapsedMs(batch) * 1e3 / buffers;
	}

	// zero-copy entry points: the host writes the next input in place and reads the result in place (here: one pass over each);
	// `depth` buffers in flight (the engine has 3 slots)
	double usZero[2] = { 0.0, 0.0 };
	double checksum = 0.0;
	for (int depth = 2; depth <= 3; depth++)
	{
		std::vector<int> tickets;
		for (int k = 0; k < depth - 1; k++)
		{
			float* slot = NA_BatchNextInput(batch, (size_t)frames);
			CHECK(slot != nullptr);
			std::memcpy(slot, in.data(), count * sizeof(float));
			const int t = NA_BatchSubmit(batch, nullptr, (size_t)frames);
			CHECK(t >= 0);
			tickets.push_back(t);
		}
		t0 = Now();
		for (int i = 0; i < buffers; i++)
		{
			float* slot = NA_BatchNextInput(batch, (size_t)frames);
			CHECK(slot != nullptr);
			std::memcpy(slot, in.data(), count * sizeof(float)); // the producer's write
			const int next = NA_BatchSubmit(batch, nullptr, (size_t)frames);
			CHECK(next >= 0);
			tickets.push_back(next);
			const int done = tickets.front();
			tickets.erase(tickets.begin());
			CHECK(NA_BatchCollect(batch, done, nullptr) == 0);
			const float* y = NA_BatchOutputView(batch, done);
			CHECK(y != nullptr);
			for (size_t k = 0; k < count; k += 4096) checksum += y[k]; // the consumer's read (sparse: a real consumer reads all of it)
		}
		for (int t : tickets) CHECK(NA_BatchCollect(batch, t, nullptr) == 0);
		usZero[depth - 2] = (Now() - t0) * 1e6 / buffers;
	}

	std::printf("{\"streams\": %d, \"frames\": %d, \"buffers\": %d, \"gate\": %d, \"eq\": %d, \"eq_sections\": %d, \"meter\": %d, \"meter_window\": %d, \"meter_windows_read\": %llu, \"tuner\": %d, \"tuner_hop\": %d, \"tuner_stagger\": %d, \"tuner_evaluations_read\": %llu, \"mix_groups\": %d, \"mix_dry\": %d, \"reverb\": %d, \"reverb_taps\": %d, \"reverb_irs\": %d, \"reverb_device_bytes\": %lld, \"reverb_load_irs_ms\": %.1f, \"reverb_input_spectrum_bytes_per_buffer\": %lld, \"reverb_distinct_ir_spectrum_bytes\": %lld, \"delay\": %d, \"delay_samples\": %d, \"delay_device_bytes\": %lld, \"comp\": %d, \"mod\": %d, \"mod_voices\": %d, \"mod_feedback\": %.3g, \"mod_device_bytes\": %lld, \"pipelined_period_us\": {\"p50\": %.1f, \"p99\": %.1f, \"max\": %.1f}, \"us_per_buffer_copying_between_marks\": %.3f, \"us_per_buffer_zero_copy\": %.3f, \"us_per_buffer_zero_copy_3_in_flight\": %.3f, \"us_per_buffer_copying\": %.3f, "
		"\"blocking_latency_us\": {\"p50\": %.1f, \"p99\": %.1f, \"max\": %.1f}, \"in_place_latency_us\": {\"p50\": %.1f, \"p99\": %.1f}, \"registered_blocking_latency_us\": {\"p50\": %.1f, \"p99\": %.1f}, \"checksum\": %.6g}\n",
		streams, frames, buffers, gate, eq, eq >= 0 ? eqSections : 0, meter, meter >= 0 ? meterWindow : 0, meterWindows, tuner, tuner >= 0 ? tunerHop : 0, tunerStagger ? 1 : 0, tunerEvaluations, mixGroups, mixGroups >= 0 && mixDry ? 1 : 0, reverb, reverb >= 0 ? reverbTaps : 0, reverb > 0 ? reverbIRs : 0, reverbBytes, reverbLoadMs, reverbInputSpectrumBytes, reverbDistinctIRBytes, delay, delay >= 0 ? delaySamples : 0, delayBytes, comp, mod, mod >= 0 ? modVoices : 0, mod >= 0 ? modFb : 0.0, modBytes, periodP50, periodP99, periodMax, usMarked, usZero[0], usZero[1], usCopy, lat[lat.size() / 2], lat[(size_t)(lat.size() * 0.99)], lat.back(), latInPlace[latInPlace.size() / 2], latInPlace[(size_t)(latInPlace.size() * 0.99)], latReg[latReg.size() / 2], latReg[(size_t)(latReg.size() * 0.99)], checksum);
	NA_BatchDestroy(batch);
	DeleteModel(model);
	DeleteLoader(loader);
	return 0;
}
