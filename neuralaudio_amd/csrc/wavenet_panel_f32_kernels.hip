// wavenet_panel_f32_kernels.hip -- exact f32 arithmetic for WaveNets with layer arrays of 129 .. 256 channels, on request
// (NeuralModelLoader::SetWaveNetExactF32, NA_SetWaveNetExactF32; family WN_FAMILY_WIDE_F32, wavenet_choice.h).  Only that option loads
// such a model; up to 128 channels it runs WaveNetWideF32Kernel (wavenet_wide_f32_kernels.hip), whose design rests on a whole matrix
// fitting LDS beside the block image.  From 129 channels on it does not (256 x 256 floats = 256 KB), so this kernel brings a matrix
// through LDS in k-panels and keeps what a lane owns in registers.  Same contract: every mat-mul on v_mfma_f32_16x16x4_f32 with plain
// f32 operands, no clamp, no saturation, no range-event word, NaN / inf inputs not cleaned.  Same natural-layout table (WnPrewarmLayer),
// same tap-major weight copy, same stream state (f32 quads, tile layout): prewarm / ring fill / reset / snapshots are shared.
//
//   workgroup = one stream = 512 threads = 8 waves, a block of at most 64 frames.  Wave w owns the 16-frame tile w & 3 and the row
//   half w >> 2: of a matrix with nbo 16-row blocks, hb = ceil(nbo / 2), the row blocks (w >> 2) hb .. + hb - 1 -- at most 8 accumulator
//   quads per lane at 256 channels.  M = 16 output channels, N = 16 frames, K = 4 input channels per MFMA.
//   Operand mapping (the wide kernel's): MFMA step s (0 .. 3) of the 16-channel k block kb takes input channel 16 kb + 4 q + s from
//   lane group q = lane >> 4.  B of step s = component s of the quad the lane holds for its own frame; A of the four steps = ONE
//   16-byte LDS read of the image lane (i = lane & 15, q) = W[16 rb + i][16 kb + 4 q .. + 3].
//   Registers: the residual stream xr[] and the head accumulator head[] of the wave's own (rows, frames) positions, at most 8 quads each.
//     A lane only ever updates its own positions; the layout follows the array's width and changes only where everything passes
//     through LDS anyway (rechannel, head rechannel).
//   LDS: ONE B image IMG[G <= 64][64 frames] float4 (<= 64 KB): the layer input X while the conv taps run (in-block taps read it at
//     frame - shift per lane; taps that reach in front of the block read the ring in HBM), z while the 1x1 runs, the head accumulator for
//     the head rechannel, the previous array's output for the next array's rechannel.  Each change of content sits between two LDS barriers.
//     Weights: k-panels of 32 input channels, [<= 16 row blocks][2 k blocks][64 lanes] float4 (<= 32 KB), two buffers: the next panel is
//     gathered from global memory into registers (StageLoad) while the current one feeds the MFMAs, and committed behind ONE LDS-only
//     barrier per panel.  A 256 x 256 matrix = 8 panels of 64 MFMAs per wave.  Total 64 + 2 x 32 KB + the condition row = 131 328 bytes.
//   One template over NBH = row blocks per wave, instantiated for 6 / 8 (<= 192 / 256 channels): the layer walk is the same.
//
// Sum order, per accumulator: taps ascending, then k blocks ascending (panel by panel), then s ascending, the MFMA's own four-way sum
// inside -- a function of the model alone: a sample's bits do not depend on the block length or on how the signal is cut into calls.
// The unit is compiled with -ffp-contract=off like the wide f32 unit.
//
// Calls longer than 64 frames are ordered launches on the batch's stream (wavenet_launch.h LaunchWaveNetExactF32), never a loop in
// here: a launch writes ring positions pos0 .. pos0 + n - 1 and reads pos0 - history .. pos0 - 1, which AddRing's history + 128 keeps apart.
#include "device_once.h"

#include <hip/hip_runtime.h>

#include "wavenet_dev.h"
#include "wavenet_launch.h"

namespace na
{
	namespace pf
	{
		constexpr int FRAMES = WN_PANEL_MAX_FRAMES;
		constexpr int NTHREADS = 512;
		constexpr int RING_SLACK = WN_MAX_FRAMES; // wavenet_plan.cpp AddRing: R = roundup16(history) + 128
		typedef float f32x4 __attribute__((ext_vector_type(4)));
		typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4))); // a 16-byte load from a 4-byte aligned address

		// Activation.h:83-91; the expressions of wf::Activate (wavenet_wide_f32_kernels.hip)
		__device__ __forceinline__ float FastTanh(float x)
		{
			const float ax = fabsf(x);
			const float x2 = x * x;
			return (x * (2.45550750702956f + 2.45550750702956f * ax + (0.893229853513558f + 0.821226666969744f * ax) * x2)) *
				__builtin_amdgcn_rcpf(2.44506634652299f + (2.44506634652299f + x2) * (ax + 0.814642734961073f * x2));
		}
		__device__ __forceinline__ float Activate(float v, int act)
		{
			if (act == 1) return v > 0.0f ? v : 0.01f * v;                                                                       // Activation.h:110-118
			if (act == 2) return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(v * 2.885390081777927f) + 1.0f); // StdMath tanh
			return FastTanh(v);
		}

		// float4 index of (ring position p, channel group g) in the tile layout with G channel groups: ((p >> 4) G + g) 16 + (p & 15)
		__device__ __forceinline__ size_t RingQuad(int ringOffF4, int G, int p, int g) { return (size_t)ringOffF4 + (size_t)(((p >> 4) * G + g) * 16 + (p & 15)); }

		struct Args
		{
			const WnPrewarmLayer* layers;
			int numLayers;
			const float* w; // flat weights, reference order, layer convs tap-major
			const int* ringOffF4;
			const int* ringFrames;
			const int* ringG;
			int nrings, stateF4, maxC;
			float headScale;
			float* state;
			const int* slots; // nullptr: contiguous (slot0 + i, row0 + i)
			const int* rows;
			int slot0, row0;
		};

		// workgroup barrier that orders LDS traffic only: the weight loads of the next panel stay in flight across it.  (No thread of the
		// block reads global memory another one wrote in this launch: ring stores are history for LATER launches.)
		__device__ __forceinline__ void LdsBarrier()
		{
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
			__builtin_amdgcn_s_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
		}

		// a row-major [cout x cin] matrix at w[off] (tap k of a layer conv at wconv is the matrix at wconv + k cout cin), nbo row blocks
		struct MatRef
		{
			int off, cout, cin, nbo;
		};
		template <int NBH>
		struct StagedRegs
		{
			static constexpr int ITEMS = (2 * NBH * 2 * 64) / NTHREADS; // NBH / 2 quads per thread
			f32x4 v[ITEMS];
		};
		// panel p = k blocks 2 p, 2 p + 1.  Item idx = (block rb 2 + kbl, lane (i, q)) <- W[16 rb + i][16 (2 p + kbl) + 4 q .. + 3], zero
		// outside the matrix: the wide kernel's gather
		template <int NBH>
		__device__ __forceinline__ void StageLoad(StagedRegs<NBH>& r, const float* __restrict__ w, const MatRef& m, int p)
		{
#pragma unroll
			for (int it = 0; it < StagedRegs<NBH>::ITEMS; it++)
			{
				const int idx = threadIdx.x + it * NTHREADS;
				const int lane = idx & 63, blk = idx >> 6, rb = blk >> 1, kb = 2 * p + (blk & 1);
				const int o = 16 * rb + (lane & 15), c0 = 16 * kb + 4 * (lane >> 4);
				const bool on = rb < m.nbo && o < m.cout && c0 < m.cin;
				const float* src = w + m.off + (size_t)o * m.cin + c0;
				f32x4 v = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
				if (on && c0 + 3 < m.cin)
				{
					const f32x4u t = *reinterpret_cast<const f32x4u*>(src);
					v = f32x4{ t.x, t.y, t.z, t.w };
				}
				else if (on)
				{
					v.x = src[0];
					v.y = (c0 + 1 < m.cin) ? src[1] : 0.0f;
					v.z = (c0 + 2 < m.cin) ? src[2] : 0.0f;
				}
				r.v[it] = v;
			}
		}
		template <int NBH>
		__device__ __forceinline__ void StageCommit(f32x4* buf, const StagedRegs<NBH>& r, int nbo)
		{
#pragma unroll
			for (int it = 0; it < StagedRegs<NBH>::ITEMS; it++)
			{
				const int idx = threadIdx.x + it * NTHREADS;
				if (idx < nbo * 2 * 64) buf[idx] = r.v[it];
			}
		}

		// acc[r] += M[16 (rb0 + r) .. + 16][the panel's kbs k blocks] * b[kbl] for the wave's hb row blocks from rb0 on (below nbo); k block
		// by k block, in groups of four row blocks: consecutive MFMAs write different accumulators, a group's four LDS quads are all of
		// the panel that is in registers at a time (the scheduling barrier keeps the reads of the whole unrolled panel where they are)
		template <int NBH>
		__device__ __forceinline__ void PanelMfma(const f32x4* buf, int rb0, int hb, int nbo, int kbs, int lane, const f32x4 (&b)[2], f32x4 (&acc)[NBH])
		{
#pragma unroll
			for (int kbl = 0; kbl < 2; kbl++)
			{
				if (kbl >= kbs) break;
#pragma unroll
				for (int r0 = 0; r0 < NBH; r0 += 4)
				{
					if (r0 >= hb) break;
					f32x4 a[4];
#define NA_PF_ON(r) (r0 + (r) < NBH && r0 + (r) < hb && rb0 + r0 + (r) < nbo)
#pragma unroll
					for (int r = 0; r < 4; r++)
						if (NA_PF_ON(r)) a[r] = buf[((rb0 + r0 + r) * 2 + kbl) * 64 + lane];
#pragma unroll
					for (int r = 0; r < 4; r++)
						if (NA_PF_ON(r)) acc[(r0 + r) % NBH] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].x, b[kbl].x, acc[(r0 + r) % NBH], 0, 0, 0);
#pragma unroll
					for (int r = 0; r < 4; r++)
						if (NA_PF_ON(r)) acc[(r0 + r) % NBH] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].y, b[kbl].y, acc[(r0 + r) % NBH], 0, 0, 0);
#pragma unroll
					for (int r = 0; r < 4; r++)
						if (NA_PF_ON(r)) acc[(r0 + r) % NBH] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].z, b[kbl].z, acc[(r0 + r) % NBH], 0, 0, 0);
#pragma unroll
					for (int r = 0; r < 4; r++)
						if (NA_PF_ON(r)) acc[(r0 + r) % NBH] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].w, b[kbl].w, acc[(r0 + r) % NBH], 0, 0, 0);
#undef NA_PF_ON
					__builtin_amdgcn_sched_barrier(0);
				}
			}
		}

		__device__ __forceinline__ f32x4 Load4(const float* __restrict__ w, int off, int c0, int count)
		{
			f32x4 v;
			v.x = (c0 + 0 < count) ? w[off + c0 + 0] : 0.0f;
			v.y = (c0 + 1 < count) ? w[off + c0 + 1] : 0.0f;
			v.z = (c0 + 2 < count) ? w[off + c0 + 2] : 0.0f;
			v.w = (c0 + 3 < count) ? w[off + c0 + 3] : 0.0f;
			return v;
		}

		constexpr size_t LdsBytes(int nbh, int gq) { return (size_t)gq * FRAMES * 16 + (size_t)2 * (2 * nbh) * 2 * 64 * 16 + FRAMES * sizeof(float); }

		template <int NBH>
		__global__ void __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(2))) WaveNetPanelF32Kernel(const Args a, const float* __restrict__ in, float* __restrict__ out,
			long inStride, long outStride, int n)
		{
			constexpr int PANEL = 2 * NBH * 2 * 64; // float4 of one panel buffer
			const f32x4 ZERO = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
			extern __shared__ __attribute__((aligned(16))) float lds[];
			const int GQ = (a.maxC + 3) / 4;                              // channel groups of the widest array
			f32x4* IMG = reinterpret_cast<f32x4*>(lds);                   // [GQ][FRAMES]: the one B image
			f32x4* pan0 = IMG + (size_t)GQ * FRAMES;                      // [2][PANEL]
			float* condL = reinterpret_cast<float*>(pan0 + 2 * PANEL);    // [FRAMES]
			int par = 0; // panels so far (workgroup-uniform)
			const int tid = threadIdx.x;
			const int f = tid & (FRAMES - 1), cq = tid >> 6;              // gather / ring role: frame f, channel groups cq, cq + 8, ..
			const int lane = tid & 63, wave = tid >> 6;                   // mat-mul role
			const int rh = wave >> 2;                                     // the wave's row half
			const int j = lane & 15, q = lane >> 4, tf = 16 * (wave & 3) + j; // the lane's frame
			const int sidx = blockIdx.x;
			const int slot = a.slots ? a.slots[sidx] : a.slot0 + sidx;
			const int row = a.slots ? a.rows[sidx] : a.row0 + sidx;
			float* st = a.state + (size_t)slot * (size_t)a.stateF4 * 4;
			f32x4* stq = reinterpret_cast<f32x4*>(st);
			int* header = reinterpret_cast<int*>(st);
			if (cq == 0) condL[f] = (f < n) ? in[(size_t)row * inStride + f] : 0.0f; // WaveNet.h:770 (input -> condition), as it is
			// the lane's own positions: row block rb = rh hb + r of the current array's layout, channel group 4 rb + q, frame tf
			f32x4 xr[NBH], head[NBH];
#pragma unroll
			for (int r = 0; r < NBH; r++)
			{
				xr[r] = ZERO;
				head[r] = ZERO; // :772 headArray.SetZero()
			}
			__syncthreads();
			const float cond = condL[tf];

			const float* __restrict__ w = a.w;
			StagedRegs<NBH> pre;  // the next panel, under way while the current one runs
			bool havePre = false; // (workgroup-uniform)
			// v[] (layout of nbl row blocks) -> IMG, each lane its own positions below Gl groups
			auto putImage = [&](const f32x4 (&v)[NBH], int nbl, int Gl) {
				const int hb = (nbl + 1) / 2;
#pragma unroll
				for (int r = 0; r < NBH; r++)
				{
					const int g = 4 * (rh * hb + r) + q;
					if (r < hb && rh * hb + r < nbl && g < Gl) IMG[g * FRAMES + tf] = v[r];
				}
			};
			// acc = M * IMG[., own frame]: a mat-mul of its own (rechannel, head rechannel), panel by panel, nothing under way before it.
			// The first panel's barrier also publishes what the caller put into IMG.
			auto matMulOwnFrame = [&](const MatRef& m, int Gin, f32x4 (&acc)[NBH]) {
				const int nbk = (m.cin + 15) / 16, hb = (m.nbo + 1) / 2;
#pragma unroll
				for (int r = 0; r < NBH; r++) acc[r] = ZERO;
				for (int p = 0; 2 * p < nbk; p++)
				{
					f32x4* buf = pan0 + (par++ & 1) * PANEL;
					StageLoad<NBH>(pre, w, m, p);
					StageCommit<NBH>(buf, pre, m.nbo);
					LdsBarrier();
					f32x4 b[2];
#pragma unroll
					for (int kbl = 0; kbl < 2; kbl++)
					{
						const int g = 4 * (2 * p + kbl) + q;
						b[kbl] = (2 * p + kbl < nbk && g < Gin) ? IMG[g * FRAMES + tf] : ZERO;
					}
					PanelMfma<NBH>(buf, rh * hb, hb, m.nbo, nbk - 2 * p, lane, b, acc);
				}
			};
			for (int li = 0; li < a.numLayers; li++)
			{
				const WnPrewarmLayer L = a.layers[li];
				if (L.kind == 0)
				{
					const int cin = L.cin; // == cout
					const int Gl = (cin + 3) / 4, nb = (cin + 15) / 16, hb = (nb + 1) / 2, P = (nb + 1) / 2;
					if (L.rechannel >= 0)
					{
						// rechannel (:637): array 0 from the condition (input_size == 1), later arrays from the previous array's output (in xr)
						if (li == 0 && L.rech_in == 1)
						{
#pragma unroll
							for (int r = 0; r < NBH; r++)
							{
								const int g = 4 * (rh * hb + r) + q;
								xr[r] = (r < hb && rh * hb + r < nb && g < Gl) ? Load4(w, L.rechannel, 4 * g, cin) * cond : ZERO;
							}
						}
						else
						{
							const int nbk = (L.rech_in + 15) / 16, Gin = (L.rech_in + 3) / 4;
							LdsBarrier(); // every wave is past the head mat-mul's reads of IMG
							putImage(xr, nbk, Gin);
							f32x4 acc[NBH];
							matMulOwnFrame(MatRef{ L.rechannel, cin, L.rech_in, nb }, Gin, acc);
#pragma unroll
							for (int r = 0; r < NBH; r++)
							{
								const int g = 4 * (rh * hb + r) + q;
								xr[r] = (r < hb && rh * hb + r < nb && g < Gl) ? acc[r] : ZERO;
							}
						}
						havePre = false;
					}
					const int R = a.ringFrames[L.ring_id], G = a.ringG[L.ring_id], roff = a.ringOffF4[L.ring_id];
					const int pos0 = header[L.ring_id];
					const int K = L.ksize, T = (K + 1) * P; // panels of the layer: K taps, then the 1x1
					// the ring part of panel t's B operands (a tap whose frame lies in front of the block): fetched one panel ahead
					auto ringQuads = [&](int t, f32x4 (&h)[2]) {
						const int mi = t / P, p = t - mi * P;
						const int src = tf - L.dilation * (K - 1 - mi);
						int pr = pos0 + src; // src >= -(R - RING_SLACK): one wrap
						if (pr < 0) pr += R;
#pragma unroll
						for (int kbl = 0; kbl < 2; kbl++)
						{
							const int g = 4 * (2 * p + kbl) + q;
							h[kbl] = (mi < K && src < 0 && g < Gl) ? stq[RingQuad(roff, G, pr, g)] : ZERO;
						}
					};
					f32x4 acc[NBH];
#pragma unroll
					for (int r = 0; r < NBH; r++) acc[r] = ZERO;
					f32x4 hNext[2], hCur[2];
					ringQuads(0, hNext);
					// one panel: commit it, set the next one out, barrier, B operands, MFMAs
					auto panel = [&](int t) {
						const int mi = t / P, p = t - mi * P;
						f32x4* buf = pan0 + (par++ & 1) * PANEL; // read two panels ago: every wave is past it (the last panel's barrier)
						if (!havePre) StageLoad<NBH>(pre, w, MatRef{ mi < K ? L.wconv + mi * cin * cin : L.w1, cin, cin, nb }, p);
						StageCommit<NBH>(buf, pre, nb);
						// the next panel sets out now: of this layer, or the first tap of the next layer of the same array
						havePre = false;
						hCur[0] = hNext[0];
						hCur[1] = hNext[1];
						if (t + 1 < T)
						{
							const int mn = (t + 1) / P, pn = (t + 1) - mn * P;
							StageLoad<NBH>(pre, w, MatRef{ mn < K ? L.wconv + mn * cin * cin : L.w1, cin, cin, nb }, pn);
							havePre = true;
							ringQuads(t + 1, hNext);
						}
						else if (li + 1 < a.numLayers)
						{
							const WnPrewarmLayer N = a.layers[li + 1];
							if (N.kind == 0 && N.rechannel < 0)
							{
								StageLoad<NBH>(pre, w, MatRef{ N.wconv, N.cin, N.cin, (N.cin + 15) / 16 }, 0);
								havePre = true;
							}
						}
						if (t == 0)
						{
							LdsBarrier(); // every wave is past its reads of what IMG held (z of the last layer, a rechannel's input)
							putImage(xr, nb, Gl);
						}
						LdsBarrier(); // the panel is staged; IMG is complete for every frame
						if (t == 0)
						{
							// the layer input of this block -> its ring (history for LATER launches: only the last R - 128 frames can be read back)
							int pw = pos0 + f;
							if (pw >= R) pw -= R;
							if (f < n && f >= n - (R - RING_SLACK))
								for (int g = cq; g < Gl; g += NTHREADS / FRAMES) stq[RingQuad(roff, G, pw, g)] = IMG[g * FRAMES + f];
						}
						// tap mi reads the frame d (K - 1 - mi) back: IMG inside the block, the ring before it; the 1x1 reads z of the own frame
						const int src = mi < K ? tf - L.dilation * (K - 1 - mi) : tf;
						f32x4 b[2];
#pragma unroll
						for (int kbl = 0; kbl < 2; kbl++)
						{
							const int g = 4 * (2 * p + kbl) + q;
							b[kbl] = (2 * p + kbl < nb && g < Gl) ? (src >= 0 ? IMG[g * FRAMES + src] : hCur[kbl]) : ZERO;
						}
						PanelMfma<NBH>(buf, rh * hb, hb, nb, nb - 2 * p, lane, b, acc);
					};
					for (int t = 0; t < K * P; t++) panel(t);
					// bias + mix-in (:288-289, :471), activation (:473-480), head accumulate (:482) -- in the lanes that hold the results;
					// z replaces X in IMG as the 1x1's B operand
					LdsBarrier(); // every wave has read its taps' frames of X
#pragma unroll
					for (int r = 0; r < NBH; r++)
					{
						const int g = 4 * (rh * hb + r) + q;
						if (r < hb && rh * hb + r < nb && g < Gl)
						{
							const f32x4 bc = Load4(w, L.bconv, 4 * g, cin), wm = Load4(w, L.wmix, 4 * g, cin);
							f32x4 zv;
							zv.x = (4 * g + 0 < cin) ? Activate(acc[r].x + bc.x + wm.x * cond, L.act) : 0.0f;
							zv.y = (4 * g + 1 < cin) ? Activate(acc[r].y + bc.y + wm.y * cond, L.act) : 0.0f;
							zv.z = (4 * g + 2 < cin) ? Activate(acc[r].z + bc.z + wm.z * cond, L.act) : 0.0f;
							zv.w = (4 * g + 3 < cin) ? Activate(acc[r].w + bc.w + wm.w * cond, L.act) : 0.0f;
							head[r] += zv;
							IMG[g * FRAMES + tf] = zv;
						}
						acc[r] = ZERO;
					}
					for (int t = K * P; t < T; t++) panel(t);
					// 1x1 bias + residual (:486-491); the last layer's output feeds the next array's rechannel (or nothing)
#pragma unroll
					for (int r = 0; r < NBH; r++)
					{
						const int g = 4 * (rh * hb + r) + q;
						if (r < hb && rh * hb + r < nb && g < Gl)
						{
							const f32x4 b1 = Load4(w, L.b1, 4 * g, cin);
							xr[r] += f32x4{ acc[r].x + b1.x, acc[r].y + b1.y, acc[r].z + b1.z, acc[r].w + b1.w };
						}
					}
				}
				else
				{
					// head rechannel (:658-660): becomes the next array's head accumulator (:785-789) or, for the last array, the output.
					// K = 1: a dense layer on the frame's own head column (matrix pipe).  K > 1 (a conv head, on the LAST array of up to 64
					// channels: ValidateWaveNetDesc): the head accumulator has its own ring -- publish, then every tap reads the frame
					// (K-1-k) head_dilation back, from IMG inside the block and from the ring before it (thread = frame, f32 VALU).
					const bool last = (li == a.numLayers - 1);
					const int Gin = (L.cin + 3) / 4, nbk = (L.cin + 15) / 16, nbo = (L.cout + 15) / 16, Gout = (L.cout + 3) / 4;
					LdsBarrier(); // every wave is past the last 1x1's reads of z
					putImage(head, nbk, Gin);
					havePre = false;
					if (L.ksize > 1)
					{
						__syncthreads();
						const int R = a.ringFrames[L.ring_id], G = a.ringG[L.ring_id], roff = a.ringOffF4[L.ring_id];
						const int pos0 = header[L.ring_id];
						int pw = pos0 + f;
						if (pw >= R) pw -= R;
						if (f < n && f >= n - (R - RING_SLACK))
							for (int g = cq; g < Gin; g += NTHREADS / FRAMES) stq[RingQuad(roff, G, pw, g)] = IMG[g * FRAMES + f];
						if (cq == 0 && f < n)
						{
							float accv = (L.bconv >= 0) ? w[L.bconv] : 0.0f; // :793-798: head channel 0 is the output
							for (int k = 0; k < L.ksize; k++)
							{
								const int off = f - L.dilation * (L.ksize - 1 - k);
								int pq = pos0 + off;
								if (pq < 0) pq += R;
								for (int g = 0; g < Gin; g++)
								{
									const f32x4 hv = (off >= 0) ? IMG[g * FRAMES + off] : stq[RingQuad(roff, G, pq, g)];
									const size_t wo = (size_t)L.wconv + ((size_t)4 * g) * L.ksize + k;
									accv += w[wo] * hv.x;
									if (4 * g + 1 < L.cin) accv += w[wo + L.ksize] * hv.y;
									if (4 * g + 2 < L.cin) accv += w[wo + 2 * L.ksize] * hv.z;
									if (4 * g + 3 < L.cin) accv += w[wo + 3 * L.ksize] * hv.w;
								}
							}
							out[(size_t)row * outStride + f] = a.headScale * accv;
						}
					}
					else
					{
						f32x4 acc[NBH];
						matMulOwnFrame(MatRef{ L.wconv, L.cout, L.cin, nbo }, Gin, acc);
						const int hbo = (nbo + 1) / 2;
						if (last)
						{
							// row 0: row block 0 of the first row half, lane group 0
							if (rh == 0 && q == 0 && tf < n) out[(size_t)row * outStride + tf] = a.headScale * (acc[0].x + ((L.bconv >= 0) ? w[L.bconv] : 0.0f)); // :793-798
						}
						else
						{
#pragma unroll
							for (int r = 0; r < NBH; r++)
							{
								const int g = 4 * (rh * hbo + r) + q;
								f32x4 v = ZERO;
								if (r < hbo && rh * hbo + r < nbo && g < Gout)
								{
									const f32x4 bb = (L.bconv >= 0) ? Load4(w, L.bconv, 4 * g, L.cout) : ZERO;
									v = f32x4{ acc[r].x + bb.x, acc[r].y + bb.y, acc[r].z + bb.z, acc[r].w + bb.w };
									if (4 * g + 1 >= L.cout) v.y = 0.0f;
									if (4 * g + 2 >= L.cout) v.z = 0.0f;
									if (4 * g + 3 >= L.cout) v.w = 0.0f;
								}
								head[r] = v; // in the NEXT array's layout (head_size == its channels)
							}
						}
					}
				}
			}
			__syncthreads();
			// advance every ring cursor by n (ChannelHistoryBuffer::AdvanceFrames, WaveNet.h:59-65, as a true modulo ring)
			if (tid < a.nrings)
			{
				const int R = a.ringFrames[tid];
				int p = header[tid] + n;
				if (p >= R) p -= R;
				header[tid] = p;
			}
		}

		template <int NBH>
		hipError_t Launch(const Args& a, int numStreams, const float* in, float* out, long inStride, long outStride, int n, hipStream_t stream)
		{
			static PerDeviceOnce attr;
			(void)attr.Run([] { return hipFuncSetAttribute(reinterpret_cast<const void*>(&WaveNetPanelF32Kernel<NBH>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
			hipLaunchKernelGGL((WaveNetPanelF32Kernel<NBH>), dim3((unsigned)numStreams), dim3(NTHREADS), LdsBytes(NBH, (a.maxC + 3) / 4), stream, a, in, out, inStride, outStride, n);
			return hipGetLastError();
		}
	}

	hipError_t LaunchWaveNetPanelF32(const WnPrewarmLayer* layers, int numLayers, const float* weights, const int* ringOffF4, const int* ringFrames, const int* ringG,
		int nrings, int stateF4, int maxChannels, float headScale, float* state, const int* slots, const int* rows, int numStreams, int slot0, int row0,
		const float* in, float* out, long inStride, long outStride, int n, hipStream_t stream)
	{
		if (numStreams <= 0 || n <= 0) return hipSuccess;
		const WaveNetExactF32LaunchChoice c = WaveNetExactF32LaunchFor(maxChannels, false);
		if (n > c.maxFrames || c.panelNb == 0) return hipErrorInvalidValue;
		pf::Args a;
		a.layers = layers;
		a.numLayers = numLayers;
		a.w = weights;
		a.ringOffF4 = ringOffF4;
		a.ringFrames = ringFrames;
		a.ringG = ringG;
		a.nrings = nrings;
		a.stateF4 = stateF4;
		a.maxC = maxChannels;
		a.headScale = headScale;
		a.state = state;
		a.slots = slots;
		a.rows = rows;
		a.slot0 = slot0;
		a.row0 = row0;
		// LDS at the widest model of each instantiation: 192 channels 98 560, 256: 131 328 bytes (of 163 840)
		if (c.panelNb == 12) return pf::Launch<6>(a, numStreams, in, out, inStride, outStride, n, stream);
		return pf::Launch<8>(a, numStreams, in, out, inStride, outStride, n, stream);
	}
}
