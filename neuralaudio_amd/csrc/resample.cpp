// resample.cpp -- host part of batch resampling (resample.h): the plan of a rate pair, the prototype filter and its
// phase-major tables, and the GpuBatch members that wrap the model launches of a call between the up and the down kernel.
#include "gpu_batch_internal.h"

#include <cmath>
#include <numeric>

namespace na
{
	ResamplePlan PlanResampling(int externalRate, int modelRate, int quantum)
	{
		if (externalRate <= 0 || modelRate <= 0)
			throw std::runtime_error("neuralaudio_amd: resampling: sample rates must be positive (" + std::to_string(externalRate) + ", " + std::to_string(modelRate) + ")");
		if (quantum == 0) quantum = kResampleDefaultQuantum;
		if (quantum != 1 && quantum != 32 && quantum != 64 && quantum != 128)
			throw std::runtime_error("neuralaudio_amd: resampling: the block quantum must be 0 (default), 1, 32, 64 or 128, not " + std::to_string(quantum));
		ResamplePlan p;
		p.externalRate = externalRate;
		p.modelRate = modelRate;
		p.quantum = quantum;
		const int g = std::gcd(externalRate, modelRate);
		const int te = modelRate / g, tm = externalRate / g; // Fc / Fe, Fc / Fm
		if (te > kResampleMaxTicks || tm > kResampleMaxTicks)
			throw std::runtime_error("neuralaudio_amd: resampling: " + std::to_string(externalRate) + " Hz against " + std::to_string(modelRate) + " Hz reduces to " +
				std::to_string(tm) + " : " + std::to_string(te) + ", beyond the supported terms (<= " + std::to_string(kResampleMaxTicks) + ")");
		p.te = te;
		p.tm = tm;
		p.identity = externalRate == modelRate;
		const int tmin = std::max(te, tm);
		p.K = kResampleT * tmin + 1;
		p.tapsUp = (p.K - 1) / te + 1;
		p.tapsDown = (p.K - 1) / tm + 1;
		if (p.identity)
		{
			p.quantum = 1;
			p.shift = 0;
			p.latency = 0;
			return p;
		}
		// S = (q - 1) * tm + pad, pad < te the ticks that make 2 * half + S a whole number of external samples
		const int base = kResampleT * tmin + (quantum - 1) * tm;
		const int pad = (te - base % te) % te;
		p.shift = (quantum - 1) * tm + pad;
		p.latency = (base + pad) / te;
		// what a call still needs of earlier calls (the derivations are in DESIGN.md 2.8): the oldest input a frame of this call reads lies
		// tapsUp + 1 + ceil((q - 1) * tm / te) samples back, the oldest model output an output sample reads tapsDown + 1 + ceil(S / tm) frames
		p.histUp = p.tapsUp + 1 + ((quantum - 1) * tm + te - 1) / te;
		p.histDown = p.tapsDown + 1 + (p.shift + tm - 1) / tm;
		return p;
	}

	void CheckResampleModelRate(int modelProcessRate, int planModelRate)
	{
		if (modelProcessRate != planModelRate)
			throw std::runtime_error("neuralaudio_amd: AddStreams: the model runs at " + std::to_string(modelProcessRate) + " Hz as loaded, the batch resamples to a model rate of " +
				std::to_string(planModelRate) + " Hz");
	}

	namespace
	{
		double BesselI0(double x)
		{
			double sum = 1.0, term = 1.0;
			const double q = x * x / 4.0;
			for (int k = 1; k < 200; k++)
			{
				term *= q / ((double)k * (double)k);
				sum += term;
				if (term < sum * 1e-17) break;
			}
			return sum;
		}
	}

	// Kaiser-windowed sinc at the common rate: pass band to (16000 / 22050) of the lower rate's Nyquist frequency, stop band from that
	// Nyquist frequency, cut-off midway, window for 100 dB.  In cycles per tick the cut-off is (1 + 16000 / 22050) / (4 * max(te, tm)),
	// whatever the rates.
	std::vector<float> ResamplePrototype(const ResamplePlan& plan)
	{
		const int tmin = std::max(plan.te, plan.tm);
		const int K = plan.K, half = kResampleT * tmin / 2;
		const double pi = 3.14159265358979323846;
		const double fc = (1.0 + 16000.0 / 22050.0) / (4.0 * (double)tmin);
		const double beta = 0.1102 * (100.0 - 8.7);
		const double i0b = BesselI0(beta);
		std::vector<float> h((size_t)K);
		for (int n = 0; n < K; n++)
		{
			const double t = (double)(n - half);
			const double x = 2.0 * fc * t;
			const double sinc = (n == half) ? 1.0 : std::sin(pi * x) / (pi * x);
			const double r = t / (double)half;
			const double w = BesselI0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
			h[(size_t)n] = (float)(2.0 * fc * sinc * w);
		}
		// (exactly symmetric: both halves are rounded from the same doubles only if they are the same doubles)
		for (int n = 0; n < half; n++) h[(size_t)(K - 1 - n)] = h[(size_t)n];
		return h;
	}

	void ResampleTables(const ResamplePlan& plan, const std::vector<float>& h, std::vector<float>& up, std::vector<float>& down)
	{
		auto fill = [&](std::vector<float>& table, int period, int taps) {
			table.assign((size_t)period * (size_t)taps, 0.0f);
			for (int phase = 0; phase < period; phase++)
				for (int t = 0; t < taps; t++)
				{
					const long idx = (long)phase + (long)t * period;
					if (idx < (long)h.size()) table[(size_t)phase * (size_t)taps + (size_t)t] = h[(size_t)idx];
				}
		};
		fill(up, plan.te, plan.tapsUp);
		fill(down, plan.tm, plan.tapsDown);
	}

	// ------------------------------------------------------------------------------------------------------------------ GpuBatch

	bool GpuBatch::Resamples() const { return resample && !resample->plan.identity; }

	const ResamplePlan& GpuBatch::ResamplingPlan() const
	{
		if (!resample) throw std::runtime_error("neuralaudio_amd: the batch does not resample (NA_BatchSetResampling was not called)");
		return resample->plan;
	}

	long long GpuBatch::ResampleSamplesTaken() const { return resample ? resample->E : -1; }

	void GpuBatch::SetResampling(int externalRate, int modelRate, int quantum, int maxFrames)
	{
		CheckUsable();
		if (HasDryMixGroup())
			throw std::runtime_error("neuralaudio_amd: SetResampling: a mix group with a DRY tap exists (the rows of a resampling batch lag the input by the resampler's latency)");
		if (!streams.empty() || !groups.empty())
			throw std::runtime_error("neuralaudio_amd: SetResampling: the batch already has streams (it is a set-up call, before the first AddStreams)");
		if (maxFrames < 1) throw std::runtime_error("neuralaudio_amd: SetResampling: maxFrames must be >= 1");
		std::unique_ptr<ResampleState> rs(new ResampleState());
		rs->plan = PlanResampling(externalRate, modelRate, quantum);
		const ResamplePlan& p = rs->plan;
		if (!p.identity)
		{
			// the longest piece whose two windows (history ++ the piece's samples) fit the stages' LDS window
			int piece = std::min(2048, kResampleWindowFloats - p.histUp);
			while (piece >= 1 && (long long)p.histDown + ((long long)piece * p.te) / p.tm + p.quantum + 1 > kResampleWindowFloats) piece--;
			if (piece < 1)
				throw std::runtime_error("neuralaudio_amd: SetResampling: the filter of " + std::to_string(externalRate) + " Hz against " + std::to_string(modelRate) +
					" Hz (" + std::to_string(p.tapsUp) + " / " + std::to_string(p.tapsDown) + " taps) does not fit the stages' window");
			rs->pieceFrames = piece;
			CheckHip(hipSetDevice(device), "hipSetDevice");
			const std::vector<float> h = ResamplePrototype(p);
			std::vector<float> up, down;
			ResampleTables(p, h, up, down);
			CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&rs->tableUp), up.size() * sizeof(float)), "hipMalloc");
			CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&rs->tableDown), down.size() * sizeof(float)), "hipMalloc");
			CheckHip(hipMemcpy(rs->tableUp, up.data(), up.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
			CheckHip(hipMemcpy(rs->tableDown, down.data(), down.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
			rs->sizedFrames = std::min(maxFrames, piece);
			rs->modelStride = (int)(((long long)rs->sizedFrames * p.te) / p.tm) + p.quantum + 1;
		}
		resample = std::move(rs);
	}

	// Set-up side, shared by the resampling histories and the cabinet stage's rings: `block` becomes a zeroed [rows][rowFloats] block
	// whose first `keepRows` rows are the old block's.  The caller has waited for whatever reads or writes the old block.  Clear and
	// copy run on the batch stream, not the legacy stream: another shard of a multi batch may be capturing a graph on its own stream,
	// and a legacy-stream operation would have to wait for that stream.  The wait for them is bounded; if it fails the fresh block,
	// which no member owns yet, is given back -- unless the batch broke: the clear may then still be pending, and the block is left
	// alone like everything else of a broken batch (GpuBatch::IsBroken).
	void GpuBatch::GrowRowBlock(float*& block, size_t rowFloats, int keepRows, int rows, const char* mallocWhat, const char* what)
	{
		float* fresh = nullptr;
		CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&fresh), (size_t)rows * rowFloats * sizeof(float)), mallocWhat);
		hipError_t e = hipMemsetAsync(fresh, 0, (size_t)rows * rowFloats * sizeof(float), stream);
		if (e == hipSuccess && block && keepRows > 0)
			e = hipMemcpyAsync(fresh, block, (size_t)keepRows * rowFloats * sizeof(float), hipMemcpyDeviceToDevice, stream);
		if (e != hipSuccess)
		{
			(void)CountedHipFree(fresh);
			CheckHip(e, what);
		}
		try
		{
			WaitStreamBounded(stream, "hipStreamSynchronize");
		}
		catch (...)
		{
			if (!IsBroken()) (void)CountedHipFree(fresh);
			throw;
		}
		if (block) (void)CountedHipFree(block);
		block = fresh;
	}

	// set-up side (AddStreams): rows only ever grow; the histories of the rows that exist move to the new block
	void GpuBatch::EnsureResampleRows(int rows)
	{
		ResampleState& r = *resample;
		if (rows <= r.rowCapacity) return;
		const int cap = std::max(rows, r.rowCapacity * 2);
		const char* what = "resampling: growing the row blocks";
		WaitStreamBounded(stream, "hipStreamSynchronize");
		GrowRowBlock(r.histUp, (size_t)r.plan.histUp, r.rowCapacity, cap, "hipMalloc", what);
		GrowRowBlock(r.histDown, (size_t)r.plan.histDown, r.rowCapacity, cap, "hipMalloc", what);
		GrowRowBlock(r.modelIn, (size_t)r.modelStride, 0, cap, "hipMalloc", what);
		GrowRowBlock(r.modelOut, (size_t)r.modelStride, 0, cap, "hipMalloc", what);
		r.rowCapacity = cap;
	}

	// a call longer than SetResampling's maxFrames: the model-side rows grow (not real-time safe, like any first use of a longer buffer)
	void GpuBatch::EnsureResampleFrames(size_t n)
	{
		ResampleState& r = *resample;
		if (n <= (size_t)r.sizedFrames) return;
		const ResamplePlan& p = r.plan;
		WaitStreamBounded(stream, "hipStreamSynchronize");
		const int stride = (int)(((long long)n * p.te) / p.tm) + p.quantum + 1;
		for (float** block : { &r.modelIn, &r.modelOut })
			GrowRowBlock(*block, (size_t)stride, 0, r.rowCapacity, "hipMalloc", "hipMemsetAsync");
		r.sizedFrames = (int)n;
		r.modelStride = stride;
	}

	// new, recycled and prewarmed streams start from zero histories at the batch's current phase (on the batch stream)
	void GpuBatch::ZeroResampleHistories(int first, int count)
	{
		ResampleState& r = *resample;
		if (count < 1 || first < 0 || first + count > r.rowCapacity) return;
		CheckHip(hipMemsetAsync(r.histUp + (size_t)first * (size_t)r.plan.histUp, 0, (size_t)count * (size_t)r.plan.histUp * sizeof(float), stream), "hipMemsetAsync");
		CheckHip(hipMemsetAsync(r.histDown + (size_t)first * (size_t)r.plan.histDown, 0, (size_t)count * (size_t)r.plan.histDown * sizeof(float), stream), "hipMemsetAsync");
	}

	// One call of a resampling batch on `launch` (the batch stream): up kernel -> model launches over P(E1) - P(E0) frames (possibly
	// none) -> down kernel, in pieces where the call is longer than the stages' window.
	void GpuBatch::ProcessResampledOn(hipStream_t launch, const float* dIn, float* dOut, size_t n, long inStride, long outStride)
	{
		ResampleState& r = *resample;
		const ResamplePlan& p = r.plan;
		const int rows = (int)streams.size();
		if (rows > r.rowCapacity) throw std::runtime_error("neuralaudio_amd: resampling: the batch has rows without history slots");
		EnsureResampleFrames(std::min(n, (size_t)r.pieceFrames));
		for (size_t done = 0; done < n;)
		{
			const int piece = (int)std::min(n - done, (size_t)r.pieceFrames);
			const long long E0 = r.E, E1 = E0 + piece;
			const long long P0 = r.P, P1 = p.ModelFrames(E1);
			const int frames = (int)(P1 - P0);
			if (frames < 0 || frames > r.modelStride) throw std::runtime_error("neuralaudio_amd: resampling: model-side frame count out of range");
			ResampleStageArgs up;
			up.in = dIn + done;
			up.inStride = inStride;
			up.out = r.modelIn;
			up.outStride = r.modelStride;
			up.hist = r.histUp;
			up.table = r.tableUp;
			up.rows = rows;
			up.nIn = piece;
			up.nOut = frames;
			up.histLen = p.histUp;
			up.taps = p.tapsUp;
			// window index 0 is input sample E0 - histUp: frame j's newest tap sits at tick j * tm - (E0 - histUp) * te of the window
			up.tick0 = (int)(P0 * p.tm - (E0 - p.histUp) * p.te);
			up.step = p.tm;
			up.period = p.te;
			up.gain = (float)p.te;
			up.cleanNaN = 1;
			CheckHip(LaunchResampleUp(up, launch), "ResampleUpKernel");
			if (frames > 0) LaunchModelsOn(launch, r.modelIn, r.modelOut, (size_t)frames, r.modelStride, r.modelStride);
			ResampleStageArgs down;
			down.in = r.modelOut;
			down.inStride = r.modelStride;
			down.out = dOut + done;
			down.outStride = outStride;
			down.hist = r.histDown;
			down.table = r.tableDown;
			down.rows = rows;
			down.nIn = frames;
			down.nOut = piece;
			down.histLen = p.histDown;
			down.taps = p.tapsDown;
			// window index 0 is model frame P0 - histDown: output k's newest tap sits at tick k * te - S - (P0 - histDown) * tm
			down.tick0 = (int)(E0 * p.te - p.shift - (P0 - p.histDown) * p.tm);
			down.step = p.te;
			down.period = p.tm;
			down.gain = (float)p.tm;
			down.cleanNaN = 0;
			CheckHip(LaunchResampleDown(down, launch), "ResampleDownKernel");
			r.E = E1;
			r.P = P1;
			r.lastFrames = frames;
			r.lastRows = rows;
			done += (size_t)piece;
		}
	}

	int GpuBatch::DebugResampleTap(float* modelIn, float* modelOut, long long capacityPerRow)
	{
		CheckUsable();
		if (!Resamples()) throw std::runtime_error("neuralaudio_amd: DebugResampleTap: the batch does not resample");
		ResampleState& r = *resample;
		CheckHip(hipSetDevice(device), "hipSetDevice");
		Quiesce();
		if (r.lastFrames > capacityPerRow) throw std::runtime_error("neuralaudio_amd: DebugResampleTap: " + std::to_string(r.lastFrames) + " frames per row, capacity " + std::to_string(capacityPerRow));
		if (r.lastFrames > 0 && r.lastRows > 0)
		{
			const size_t width = (size_t)r.lastFrames * sizeof(float);
			if (modelIn) CheckHip(hipMemcpy2D(modelIn, width, r.modelIn, (size_t)r.modelStride * sizeof(float), width, (size_t)r.lastRows, hipMemcpyDeviceToHost), "hipMemcpy2D");
			if (modelOut) CheckHip(hipMemcpy2D(modelOut, width, r.modelOut, (size_t)r.modelStride * sizeof(float), width, (size_t)r.lastRows, hipMemcpyDeviceToHost), "hipMemcpy2D");
		}
		return r.lastFrames;
	}
}
