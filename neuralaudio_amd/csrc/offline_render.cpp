// offline_render.cpp -- planner and runner of NA_RenderOffline (offline_render.h; the exactness argument and the cost model: DESIGN.md 2.6).
//
// Layout.  Every row of the segment batch processes the same n = lead + L frames per pass.  Segment g of a WaveNet job reads the
// input [g L, g L + n) and keeps the outputs [g L + lead, g L + n) -- segment 0 has no lead-in and keeps [0, n) -- so the kept parts
// tile the signal and every segment after the first has `lead` >= H samples of genuine input in front of what it keeps.  A job's
// segments are dealt to its R rows pass by pass (pass p runs segments p R .. p R + R - 1); rows of a later pass simply continue from
// the state the previous segment left, which the lead-in flushes like a prewarm.  A recurrent job is one row that walks its signal n
// samples per pass with its state carried over: the sequential run itself.
#include "offline_render.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <stdexcept>
#include <thread>

#include "gpu_batch.h"
#include "resample.h"

namespace na
{
	namespace
	{
		constexpr double kPassBudgetMs = 250.0;  // estimated device time of one pass (far below the default wait limit of 2000 ms)
		constexpr double kPassOverheadMs = 0.2;  // host round trip, row table, gather / scatter of a pass

		long long RoundUp(long long v, long long m) { return (v + m - 1) / m * m; }
		long long CeilDivLL(long long a, long long b) { return (a + b - 1) / b; }

		struct JobFacts
		{
			long long T = 0;
			int H = -1; // -1: recurrent
			double cost = 1.0;
		};

		// device allocations of one render; left alone when the batch broke (a kernel may still write them, see GpuBatch::IsBroken)
		struct DeviceBuffers
		{
			const GpuBatch* batch = nullptr;
			std::vector<void*> ptrs;
			hipStream_t stream = nullptr;
			template <typename T>
			T* Alloc(size_t count)
			{
				void* p = nullptr;
				CheckHip(CountedHipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)), "hipMalloc (offline render)");
				ptrs.push_back(p);
				return (T*)p;
			}
			~DeviceBuffers()
			{
				if (batch && batch->IsBroken()) return;
				if (stream)
				{
					// (an error path may leave a copy / gather / scatter behind: wait for it within the batch's limit, else leave the buffers)
					const double ms = batch ? batch->GetWaitLimitMs() : 0.0;
					const auto end = std::chrono::steady_clock::now() + std::chrono::microseconds((long long)(ms > 0 ? ms * 1000.0 : 0));
					while (hipStreamQuery(stream) == hipErrorNotReady)
					{
						if (ms > 0 && std::chrono::steady_clock::now() > end) return;
						std::this_thread::sleep_for(std::chrono::microseconds(50));
					}
				}
				for (void* p : ptrs) (void)CountedHipFree(p);
				if (stream) (void)hipStreamDestroy(stream);
			}
		};

		int DeviceComputeUnits(int device)
		{
			int cus = 0;
			if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
			return cus;
		}
	}

	int StreamHistory(const LoadedModel& model, float quality)
	{
		if (model.subModels.empty()) throw std::runtime_error("offline render: model without submodels");
		const int idx = model.isComposite ? model.ModelIndexFromQuality(quality) : 0;
		const ModelDesc& d = *model.subModels[(size_t)idx].desc;
		if (d.kind != MODEL_WAVENET) return -1;
		int h = 0;
		for (const WnArrayCfg& a : d.wavenet.arrays)
		{
			for (size_t l = 0; l < a.kernelSizes.size(); l++) h += (a.kernelSizes[l] - 1) * a.dilations[l];
			if (a.headKernelSize > 1) h += (a.headKernelSize - 1) * a.headDilation;
		}
		return h;
	}

	RenderPlan PlanOfflineRender(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int computeUnits)
	{
		if (jobs.empty()) throw std::runtime_error("offline render: no jobs");
		const int numJobs = (int)jobs.size();
		std::vector<JobFacts> f((size_t)numJobs);
		int H = -1, numActive = 0;
		long long maxT = 0, maxTwn = 0;
		double cmax = 0.0;
		for (int j = 0; j < numJobs; j++)
		{
			if (!jobs[(size_t)j].model) throw std::runtime_error("offline render: job without a model");
			f[(size_t)j].T = (long long)jobs[(size_t)j].numSamples;
			f[(size_t)j].H = StreamHistory(*jobs[(size_t)j].model, jobs[(size_t)j].quality);
			f[(size_t)j].cost = EstimateStreamCost(*jobs[(size_t)j].model, jobs[(size_t)j].quality);
			if (f[(size_t)j].T <= 0) continue;
			numActive++;
			H = std::max(H, f[(size_t)j].H);
			maxT = std::max(maxT, f[(size_t)j].T);
			if (f[(size_t)j].H >= 0) maxTwn = std::max(maxTwn, f[(size_t)j].T);
			cmax = std::max(cmax, f[(size_t)j].cost);
		}
		if (numActive > kMaxRenderRows) throw std::runtime_error("offline render: more jobs than one segment batch holds (16384)");

		RenderPlan plan;
		plan.lead = H > 0 ? (int)RoundUp(H, WN_MAX_FRAMES) : 0;
		plan.jobRows.assign((size_t)numJobs, 0);
		plan.jobSegments.assign((size_t)numJobs, 0);
		plan.jobRecurrent.assign((size_t)numJobs, 0);
		for (int j = 0; j < numJobs; j++) plan.jobRecurrent[(size_t)j] = f[(size_t)j].H < 0;
		if (numActive == 0) return plan;

		const long long lead = plan.lead;
		const long long M = (long long)(opts.maxSamplesPerPass ? opts.maxSamplesPerPass : kDefaultMaxSamplesPerPass);
		const long long Sfull = 4LL * (computeUnits > 0 ? computeUnits : 256); // streams that fill the chip (four waves per CU)

		// row lengths to consider: the caller's segment length, else the whole signal in one row and lead + 128 * 2^k
		std::vector<long long> ns;
		if (opts.segmentSamples > 0) ns.push_back(lead + (long long)opts.segmentSamples);
		else
		{
			ns.push_back(RoundUp(maxT, WN_MAX_FRAMES));
			for (long long s = WN_MAX_FRAMES; s < 2 * maxT; s *= 2) ns.push_back(lead + s);
			// ... and the segment lengths that cut the longest WaveNet signal into a fraction or a multiple of a chip-filling batch
			if (maxTwn > lead)
				for (long long S = Sfull / 4; S <= 4 * Sfull; S *= 2) ns.push_back(lead + RoundUp(CeilDivLL(maxTwn - lead, S), WN_MAX_FRAMES));
		}

		bool haveBest = false, bestFits = false;
		double bestCost = 0.0;
		for (const long long n : ns)
		{
			const long long L = n - lead;
			std::vector<long long> G((size_t)numJobs, 0);
			bool ok = true;
			long long sumG = 0, passesRec = 1;
			int numRec = 0;
			for (int j = 0; j < numJobs; j++)
			{
				const JobFacts& x = f[(size_t)j];
				if (x.T <= 0) continue;
				if (x.H < 0)
				{
					G[(size_t)j] = 1;
					numRec++;
					passesRec = std::max(passesRec, CeilDivLL(x.T, n));
					continue;
				}
				if (x.T <= n) G[(size_t)j] = 1;
				else if (L > 0) G[(size_t)j] = CeilDivLL(x.T - lead, L);
				else ok = false;
				sumG += G[(size_t)j];
			}
			if (!ok) continue;
			const long long budget = std::min<long long>(kMaxRenderRows, std::max<long long>(numActive, M / n));
			auto rowsFor = [&](long long P) {
				long long r = numRec;
				for (int j = 0; j < numJobs; j++)
					if (f[(size_t)j].H >= 0 && G[(size_t)j] > 0) r += CeilDivLL(G[(size_t)j], P);
				return r;
			};
			long long P = passesRec;
			if (rowsFor(P) > budget)
			{
				P = std::max(P, CeilDivLL(sumG, std::max<long long>(1, budget - numRec)));
				while (rowsFor(P) > budget) P++;
			}
			double work = 0.0;
			long long rows = 0;
			std::vector<int> R((size_t)numJobs, 0);
			for (int j = 0; j < numJobs; j++)
			{
				if (G[(size_t)j] == 0) continue;
				R[(size_t)j] = (int)(f[(size_t)j].H < 0 ? 1 : CeilDivLL(G[(size_t)j], P));
				rows += R[(size_t)j];
				work += R[(size_t)j] * f[(size_t)j].cost;
			}
			// cost model: a step of 128 frames over the batch costs its streams' estimated microseconds per 1024 streams (EstimateStreamCost),
			// but never less than a batch that fills the chip -- a small batch leaves compute units idle without being any faster
			const double stepUs = std::max(work, cmax * (double)Sfull) / 1024.0;
			const double passMs = (double)CeilDivLL(n, WN_MAX_FRAMES) * stepUs / 1000.0;
			const double cost = (double)P * (passMs + kPassOverheadMs);
			const bool fits = passMs <= kPassBudgetMs;
			if (haveBest && (bestFits && !fits)) continue;
			if (haveBest && bestFits == fits && cost >= bestCost) continue;
			haveBest = true;
			bestFits = fits;
			bestCost = cost;
			plan.rowSamples = n;
			plan.stride = L;
			plan.passes = (int)P;
			plan.rows = (int)rows;
			plan.estimatedMs = cost;
			plan.segments = 0;
			for (int j = 0; j < numJobs; j++)
			{
				plan.jobRows[(size_t)j] = R[(size_t)j];
				plan.jobSegments[(size_t)j] = G[(size_t)j];
				plan.segments += G[(size_t)j];
			}
		}
		if (!haveBest) throw std::runtime_error("offline render: no segment layout fits the options");
		return plan;
	}

	RenderPlan PlanOfflineRenderOn(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device, std::string* kernelName)
	{
		if (kernelName) kernelName->clear();
		const bool haveDevice = device >= 0 && device < VisibleDeviceCount();
		RenderPlan plan = PlanOfflineRender(jobs, opts, haveDevice ? DeviceComputeUnits(device) : 0);
		if (haveDevice && kernelName && plan.rows > 0)
		{
			GpuBatch batch(device);
			int first = -1;
			for (size_t j = 0; j < jobs.size(); j++)
			{
				if (plan.jobRows[j] == 0) continue;
				const int id = batch.AddStreams(jobs[j].model, jobs[j].quality, plan.jobRows[j], false, true);
				if (first < 0) first = id;
			}
			if (first >= 0) *kernelName = batch.StreamKernelName(first);
		}
		return plan;
	}

	namespace
	{
		void CheckHostJobs(const std::vector<RenderJobDesc>& jobs)
		{
			for (const RenderJobDesc& j : jobs)
			{
				if (!j.model) throw std::runtime_error("offline render: job without a model");
				if (j.numSamples > 0 && (!j.input || !j.output)) throw std::runtime_error("offline render: job without input or output buffer");
				if (j.numSamples > 0 && j.input < j.output + j.numSamples && j.output < j.input + j.numSamples)
					throw std::runtime_error("offline render: a job's input and output overlap");
			}
		}
	}

	static void RenderSegments(GpuBatch& batch, const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device, bool deviceSignals);

	void RenderOffline(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device)
	{
		CheckHostJobs(jobs);
		GpuBatch batch(device); // throws without a device: there is no CPU fallback
		if (opts.waitLimitMs > 0) batch.SetWaitLimitMs(opts.waitLimitMs);
		RenderSegments(batch, jobs, opts, device, false);
	}

	// the segment passes of a render on `batch` (empty so far).  deviceSignals: the jobs' input / output pointers are device memory of
	// `device` (the model-rate signals of RenderOfflineAtRate) instead of host windows; nothing else differs.
	static void RenderSegments(GpuBatch& batch, const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device, bool deviceSignals)
	{
		const hipMemcpyKind inKind = deviceSignals ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
		const hipMemcpyKind outKind = deviceSignals ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
		const RenderPlan plan = PlanOfflineRender(jobs, opts, DeviceComputeUnits(device));
		if (plan.rows == 0) return;

		const int numJobs = (int)jobs.size();
		const long long n = plan.rowSamples, L = plan.stride, lead = plan.lead;
		std::vector<int> firstRow((size_t)numJobs, -1);
		for (int j = 0; j < numJobs; j++)
			if (plan.jobRows[(size_t)j] > 0)
				firstRow[(size_t)j] = batch.AddStreams(jobs[(size_t)j].model, jobs[(size_t)j].quality, plan.jobRows[(size_t)j], true, true);
		const int rows = batch.NumStreams();
		if (rows != plan.rows) throw std::runtime_error("offline render: segment batch has an unexpected row count");

		DeviceBuffers mem;
		mem.batch = &batch;
		const long long windowFloats = (long long)rows * n; // a pass's input / output windows never exceed the rows it runs
		float* dBuf = mem.Alloc<float>((size_t)windowFloats);
		float* dSig = mem.Alloc<float>((size_t)windowFloats);
		float* dOut = mem.Alloc<float>((size_t)windowFloats);
		RenderRow* dRows = mem.Alloc<RenderRow>((size_t)rows);
		CheckHip(CountedHipStreamCreateWithFlags(&mem.stream, hipStreamNonBlocking), "hipStreamCreate");
		hipStream_t rs = mem.stream;

		std::vector<RenderRow> table((size_t)rows);
		struct Window
		{
			long long inLo, inHi, outLo, outHi, sigBase, outBase;
		};
		std::vector<Window> win((size_t)numJobs);
		for (int p = 0; p < plan.passes; p++)
		{
			for (RenderRow& r : table) r = RenderRow{ 0, 0, 0, 0, 0 };
			long long sigBase = 0, outBase = 0;
			for (int j = 0; j < numJobs; j++)
			{
				Window& w = win[(size_t)j];
				w = Window{ 0, 0, 0, 0, sigBase, outBase };
				const long long T = (long long)jobs[(size_t)j].numSamples;
				const int R = plan.jobRows[(size_t)j];
				if (R == 0) continue;
				if (plan.jobRecurrent[(size_t)j])
				{
					const long long lo = std::min(T, (long long)p * n), hi = std::min(T, lo + n);
					w.inLo = w.outLo = lo;
					w.inHi = w.outHi = hi;
					table[(size_t)firstRow[(size_t)j]] = RenderRow{ sigBase, hi - lo, outBase, 0, hi - lo };
				}
				else
				{
					const long long G = plan.jobSegments[(size_t)j];
					const long long g0 = (long long)p * R, g1 = std::min(G, g0 + R);
					if (g0 < G)
					{
						w.inLo = g0 * L;
						w.outLo = g0 == 0 ? 0 : g0 * L + lead;
						w.inHi = w.outHi = std::min(T, (g1 - 1) * L + n);
						for (long long g = g0; g < g1; g++)
						{
							const long long start = g == 0 ? 0 : g * L;
							const long long valid = std::min(T, start + n) - start;
							const long long kb = g == 0 ? 0 : lead;
							table[(size_t)(firstRow[(size_t)j] + (g - g0))] =
								RenderRow{ sigBase + (start - w.inLo), valid, outBase + (start + kb - w.outLo), kb, valid };
						}
					}
				}
				sigBase += w.inHi - w.inLo;
				outBase += w.outHi - w.outLo;
			}
			// every access of the gather / scatter stays inside its buffer
			if (sigBase > windowFloats || outBase > windowFloats) throw std::runtime_error("offline render: pass window exceeds its buffer");
			for (const RenderRow& r : table)
				if (r.src < 0 || r.valid < 0 || r.valid > n || r.src + r.valid > sigBase || r.keepBegin < 0 || r.keepEnd < r.keepBegin || r.keepEnd > n ||
					(r.keepEnd > r.keepBegin && (r.dst < 0 || r.dst + (r.keepEnd - r.keepBegin) > outBase)))
					throw std::runtime_error("offline render: row table out of bounds");

			for (int j = 0; j < numJobs; j++)
			{
				const Window& w = win[(size_t)j];
				if (w.inHi > w.inLo)
					CheckHip(hipMemcpyAsync(dSig + w.sigBase, jobs[(size_t)j].input + w.inLo, (size_t)(w.inHi - w.inLo) * sizeof(float), inKind, rs),
						"hipMemcpyAsync (offline render input)");
			}
			CheckHip(hipMemcpyAsync(dRows, table.data(), table.size() * sizeof(RenderRow), hipMemcpyHostToDevice, rs), "hipMemcpyAsync (row table)");
			CheckHip(LaunchRenderGather(dRows, rows, dSig, dBuf, n, rs), "offline render gather");
			batch.WaitStreamBounded(rs, "offline render: input rows");
			// the rows are complete in device memory: the batch may run them as free-running half-batch chains (contract (b))
			batch.ProcessDevice(dBuf, dBuf, (size_t)n, (long)n, (long)n);
			batch.WaitOutputs();
			CheckHip(LaunchRenderScatter(dRows, rows, dBuf, dOut, n, rs), "offline render scatter");
			for (int j = 0; j < numJobs; j++)
			{
				const Window& w = win[(size_t)j];
				if (w.outHi > w.outLo)
					CheckHip(hipMemcpyAsync(jobs[(size_t)j].output + w.outLo, dOut + w.outBase, (size_t)(w.outHi - w.outLo) * sizeof(float), outKind, rs),
						"hipMemcpyAsync (offline render output)");
			}
			batch.WaitStreamBounded(rs, "offline render: output download");
		}
	}

	// ---------------------------------------------------------------------------------- rendering at an external rate

	namespace
	{
		struct RenderTap
		{
			float* modelIn = nullptr;
			float* modelOut = nullptr;
			long long capacity = 0;
			bool armed = false;
		};
		// Test hook only, and NOT thread-safe: one unsynchronised slot, armed by SetRenderTap and taken (and cleared) by the next
		// RenderOfflineAtRate on whatever thread.  The release library exports no way to arm it (NA_DebugSetRenderTap is compiled out
		// of its capi.cpp), so there it stays off and concurrent renders only ever copy and clear an empty slot.
		RenderTap g_renderTap;

		// the jobs as the segment machinery sees them: job i is M_i = J_i(N_i + L_i) model-rate frames (identity pairs: N_i, L_i = 0)
		struct AtRateLayout
		{
			std::vector<ResamplePlan> plans;  // one per distinct model rate
			std::vector<int> jobPlan;         // index into plans
			std::vector<long long> frames;    // M per job
		};

		AtRateLayout LayoutAtRate(const std::vector<RenderJobDesc>& jobs, int externalRate)
		{
			if (externalRate <= 0) throw std::runtime_error("offline render: the external sample rate must be positive (" + std::to_string(externalRate) + ")");
			AtRateLayout lay;
			for (const RenderJobDesc& j : jobs)
			{
				if (!j.model) throw std::runtime_error("offline render: job without a model");
				const int fm = j.model->ProcessRate();
				int k = 0;
				while (k < (int)lay.plans.size() && lay.plans[(size_t)k].modelRate != fm) k++;
				if (k == (int)lay.plans.size())
				{
					ResamplePlan p = PlanResampling(externalRate, fm, 1); // throws on a refused pair
					if (!p.identity && (OfflineResampleTile(p.tm, p.te, p.tapsUp) == 0 || OfflineResampleTile(p.te, p.tm, p.tapsDown) == 0))
						throw std::runtime_error("offline render: the filter of " + std::to_string(externalRate) + " Hz against " + std::to_string(fm) + " Hz (" +
							std::to_string(p.tapsUp) + " / " + std::to_string(p.tapsDown) + " taps) does not fit the stages' window");
					lay.plans.push_back(p);
				}
				const ResamplePlan& p = lay.plans[(size_t)k];
				lay.jobPlan.push_back(k);
				lay.frames.push_back(p.ModelFrames((long long)j.numSamples + p.latency)); // (an empty job still renders its L samples of tail)
			}
			return lay;
		}

		std::vector<RenderJobDesc> ModelRateJobs(const std::vector<RenderJobDesc>& jobs, const AtRateLayout& lay)
		{
			std::vector<RenderJobDesc> out = jobs;
			for (size_t j = 0; j < out.size(); j++)
			{
				out[j].input = nullptr;
				out[j].output = nullptr;
				out[j].numSamples = (size_t)lay.frames[j];
			}
			return out;
		}
	}

	void SetRenderTap(float* modelIn, float* modelOut, long long capacity)
	{
		g_renderTap.modelIn = modelIn;
		g_renderTap.modelOut = modelOut;
		g_renderTap.capacity = capacity;
		g_renderTap.armed = (modelIn || modelOut);
	}

	RenderPlan PlanOfflineRenderAtRateOn(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device, int externalRate,
		std::string* kernelName, ResamplePlan* firstJobPlan)
	{
		if (jobs.empty()) throw std::runtime_error("offline render: no jobs");
		const AtRateLayout lay = LayoutAtRate(jobs, externalRate);
		if (firstJobPlan) *firstJobPlan = lay.plans[(size_t)lay.jobPlan[0]];
		return PlanOfflineRenderOn(ModelRateJobs(jobs, lay), opts, device, kernelName);
	}

	void RenderOfflineAtRate(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device, int externalRate)
	{
		// the tap is for the next call only, whatever becomes of it
		const RenderTap tap = g_renderTap;
		g_renderTap = RenderTap();
		if (jobs.empty()) throw std::runtime_error("offline render: no jobs");
		// everything that can refuse the call comes before any device work
		const AtRateLayout lay = LayoutAtRate(jobs, externalRate);
		CheckHostJobs(jobs);
		const int numJobs = (int)jobs.size();
		if (numJobs > kMaxRenderRows) throw std::runtime_error("offline render: more jobs than one segment batch holds (16384)");
		if (tap.armed && lay.frames[0] > tap.capacity)
			throw std::runtime_error("offline render: the render tap holds " + std::to_string(tap.capacity) + " frames, job 0 has " + std::to_string(lay.frames[0]));

		GpuBatch batch(device); // throws without a device: there is no CPU fallback
		if (opts.waitLimitMs > 0) batch.SetWaitLimitMs(opts.waitLimitMs);

		// whole-signal device buffers: x and out at the external rate (resampled jobs only), u and v at the model rate
		DeviceBuffers mem;
		mem.batch = &batch;
		unsigned long long bytes = 0;
		for (int j = 0; j < numJobs; j++)
			bytes += 8ULL * (unsigned long long)lay.frames[(size_t)j] + (lay.plans[(size_t)lay.jobPlan[(size_t)j]].identity ? 0ULL : 8ULL * (unsigned long long)jobs[(size_t)j].numSamples);
		auto alloc = [&](long long floats) -> float* {
			try
			{
				return mem.Alloc<float>((size_t)floats);
			}
			catch (const std::exception& e)
			{
				throw std::runtime_error("offline render: no device memory for the whole-signal buffers (" + std::to_string(bytes) +
					" bytes: 8 per sample at the external rate and 8 per model-rate frame of every job): " + e.what());
			}
		};
		std::vector<float*> dX((size_t)numJobs, nullptr), dU((size_t)numJobs, nullptr), dV((size_t)numJobs, nullptr), dY((size_t)numJobs, nullptr);
		for (int j = 0; j < numJobs; j++)
		{
			const long long N = (long long)jobs[(size_t)j].numSamples, M = lay.frames[(size_t)j];
			if (M == 0) continue;
			dU[(size_t)j] = alloc(M);
			dV[(size_t)j] = alloc(M);
			if (lay.plans[(size_t)lay.jobPlan[(size_t)j]].identity) continue;
			dX[(size_t)j] = alloc(N);
			dY[(size_t)j] = alloc(N);
		}
		// the coefficient tables of every pair that resamples
		std::vector<float*> dUp(lay.plans.size(), nullptr), dDown(lay.plans.size(), nullptr);
		CheckHip(CountedHipStreamCreateWithFlags(&mem.stream, hipStreamNonBlocking), "hipStreamCreate");
		hipStream_t rs = mem.stream;
		std::vector<std::vector<float>> tables; // (alive until the uploads are waited for)
		for (size_t k = 0; k < lay.plans.size(); k++)
		{
			const ResamplePlan& p = lay.plans[k];
			if (p.identity) continue;
			tables.emplace_back();
			tables.emplace_back();
			std::vector<float>&up = tables[tables.size() - 2], &down = tables[tables.size() - 1];
			ResampleTables(p, ResamplePrototype(p), up, down);
			dUp[k] = alloc((long long)up.size());
			dDown[k] = alloc((long long)down.size());
			CheckHip(hipMemcpyAsync(dUp[k], up.data(), up.size() * sizeof(float), hipMemcpyHostToDevice, rs), "hipMemcpyAsync (resample table)");
			CheckHip(hipMemcpyAsync(dDown[k], down.data(), down.size() * sizeof(float), hipMemcpyHostToDevice, rs), "hipMemcpyAsync (resample table)");
		}

		// 1 + 2: upload x, up stage -> u (an identity job's x IS its u)
		std::vector<OfflineResampleJob> up((size_t)numJobs), down((size_t)numJobs);
		bool resamples = false;
		for (int j = 0; j < numJobs; j++)
		{
			const size_t k = (size_t)lay.jobPlan[(size_t)j];
			const ResamplePlan& p = lay.plans[k];
			const long long N = (long long)jobs[(size_t)j].numSamples, M = lay.frames[(size_t)j];
			OfflineResampleJob& a = up[(size_t)j];
			OfflineResampleJob& b = down[(size_t)j];
			a = OfflineResampleJob{ nullptr, nullptr, nullptr, 0, 0, 0, 1, 1, 1, 1, 1, 0.0f };
			b = a;
			if (M == 0) continue;
			if (p.identity)
			{
				CheckHip(hipMemcpyAsync(dU[(size_t)j], jobs[(size_t)j].input, (size_t)N * sizeof(float), hipMemcpyHostToDevice, rs), "hipMemcpyAsync (offline render input)");
				continue;
			}
			resamples = true;
			if (N > 0) CheckHip(hipMemcpyAsync(dX[(size_t)j], jobs[(size_t)j].input, (size_t)N * sizeof(float), hipMemcpyHostToDevice, rs), "hipMemcpyAsync (offline render input)");
			// u[f]: newest tap at tick f * tm, reads x at tick / te - tap, phase tick % te, gain te
			a.in = dX[(size_t)j];
			a.out = dU[(size_t)j];
			a.table = dUp[k];
			a.nIn = N;
			a.nOut = M;
			a.tick0 = 0;
			a.step = p.tm;
			a.period = p.te;
			a.taps = p.tapsUp;
			a.tile = OfflineResampleTile(a.step, a.period, a.taps);
			a.window = (int)OfflineResampleWindow(a.tile, a.step, a.period, a.taps);
			a.gain = (float)p.te;
			// out[i] = s[i + L]: newest tap at tick (i + L) * te - S, reads v at tick / tm - tap, phase tick % tm, gain tm
			b.in = dV[(size_t)j];
			b.out = dY[(size_t)j];
			b.table = dDown[k];
			b.nIn = M;
			b.nOut = N;
			b.tick0 = (long long)p.latency * p.te - p.shift;
			b.step = p.te;
			b.period = p.tm;
			b.taps = p.tapsDown;
			b.tile = OfflineResampleTile(b.step, b.period, b.taps);
			b.window = (int)OfflineResampleWindow(b.tile, b.step, b.period, b.taps);
			b.gain = (float)p.tm;
			// the newest model frame the last output reads was computed: floor(((N + L - 1) * te - S) / tm) <= J(N + L) - 1
			if (b.tick0 < 0 || (N > 0 && (b.tick0 + (N - 1) * (long long)b.step) / b.period >= M)) throw std::runtime_error("offline render: resampling layout out of range");
		}
		OfflineResampleJob* dJobs = nullptr;
		if (resamples)
		{
			void* p = nullptr;
			CheckHip(CountedHipMalloc(&p, 2 * (size_t)numJobs * sizeof(OfflineResampleJob)), "hipMalloc (offline render)");
			mem.ptrs.push_back(p);
			dJobs = (OfflineResampleJob*)p;
			CheckHip(hipMemcpyAsync(dJobs, up.data(), (size_t)numJobs * sizeof(OfflineResampleJob), hipMemcpyHostToDevice, rs), "hipMemcpyAsync (resample jobs)");
			CheckHip(hipMemcpyAsync(dJobs + numJobs, down.data(), (size_t)numJobs * sizeof(OfflineResampleJob), hipMemcpyHostToDevice, rs), "hipMemcpyAsync (resample jobs)");
			CheckHip(LaunchOfflineResampleUp(up.data(), dJobs, numJobs, rs), "OfflineResampleUpKernel");
		}
		batch.WaitStreamBounded(rs, "offline render: up stage");

		// 3: the segment machinery over u -> v, both in device memory
		std::vector<RenderJobDesc> mj = ModelRateJobs(jobs, lay);
		for (int j = 0; j < numJobs; j++)
		{
			mj[(size_t)j].input = dU[(size_t)j];
			mj[(size_t)j].output = dV[(size_t)j];
		}
		RenderSegments(batch, mj, opts, device, true);

		// 4 + 5: down stage -> out, download
		if (resamples) CheckHip(LaunchOfflineResampleDown(down.data(), dJobs + numJobs, numJobs, rs), "OfflineResampleDownKernel");
		for (int j = 0; j < numJobs; j++)
		{
			const long long N = (long long)jobs[(size_t)j].numSamples;
			if (N == 0) continue;
			const float* src = lay.plans[(size_t)lay.jobPlan[(size_t)j]].identity ? dV[(size_t)j] : dY[(size_t)j];
			CheckHip(hipMemcpyAsync(jobs[(size_t)j].output, src, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, rs), "hipMemcpyAsync (offline render output)");
		}
		if (tap.armed && lay.frames[0] > 0)
		{
			if (tap.modelIn) CheckHip(hipMemcpyAsync(tap.modelIn, dU[0], (size_t)lay.frames[0] * sizeof(float), hipMemcpyDeviceToHost, rs), "hipMemcpyAsync (render tap)");
			if (tap.modelOut) CheckHip(hipMemcpyAsync(tap.modelOut, dV[0], (size_t)lay.frames[0] * sizeof(float), hipMemcpyDeviceToHost, rs), "hipMemcpyAsync (render tap)");
		}
		batch.WaitStreamBounded(rs, "offline render: output download");
	}
}
