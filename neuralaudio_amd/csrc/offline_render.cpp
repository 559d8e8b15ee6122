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
				CheckHip(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)), "hipMalloc (offline render)");
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
				for (void* p : ptrs) (void)hipFree(p);
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

	void RenderOffline(const std::vector<RenderJobDesc>& jobs, const RenderOptionsDesc& opts, int device)
	{
		for (const RenderJobDesc& j : jobs)
		{
			if (!j.model) throw std::runtime_error("offline render: job without a model");
			if (j.numSamples > 0 && (!j.input || !j.output)) throw std::runtime_error("offline render: job without input or output buffer");
			if (j.numSamples > 0 && j.input < j.output + j.numSamples && j.output < j.input + j.numSamples)
				throw std::runtime_error("offline render: a job's input and output overlap");
		}
		GpuBatch batch(device); // throws without a device: there is no CPU fallback
		if (opts.waitLimitMs > 0) batch.SetWaitLimitMs(opts.waitLimitMs);
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
		CheckHip(hipStreamCreateWithFlags(&mem.stream, hipStreamNonBlocking), "hipStreamCreate");
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
					CheckHip(hipMemcpyAsync(dSig + w.sigBase, jobs[(size_t)j].input + w.inLo, (size_t)(w.inHi - w.inLo) * sizeof(float), hipMemcpyHostToDevice, rs),
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
					CheckHip(hipMemcpyAsync(jobs[(size_t)j].output + w.outLo, dOut + w.outBase, (size_t)(w.outHi - w.outLo) * sizeof(float), hipMemcpyDeviceToHost, rs),
						"hipMemcpyAsync (offline render output)");
			}
			batch.WaitStreamBounded(rs, "offline render: output download");
		}
	}
}
