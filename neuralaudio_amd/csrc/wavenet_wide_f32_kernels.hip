// wavenet_wide_f32_kernels.hip -- exact f32 arithmetic for WaveNets with layer arrays of 17 .. 128 channels, on request
// (NeuralModelLoader::SetWaveNetExactF32, NA_SetWaveNetExactF32; family WN_FAMILY_WIDE_F32, wavenet_choice.h).
//
// The default kernels of these widths (wavenet_generic_kernels.hip) run the three-product f16 split under the range contract of
// DESIGN.md 2.5.  This one runs every mat-mul of the model -- conv taps, 1x1, array rechannel, dense head -- on
// v_mfma_f32_16x16x4_f32 with plain f32 operands: no split, no input clamp, no saturation, no range-event word, and so none of the load
// refusals of the operand format.  NaN / inf inputs are not cleaned (the contract of the f32 frame kernel).  It walks the same
// natural-layout table (WnPrewarmLayer) over the same tap-major weight copy and keeps the generic family's stream state (f32 quads,
// tile layout), so prewarm / ring fill / reset / snapshots are shared.
//
//   workgroup = one stream = 512 threads = 8 waves; wave w owns the 16-frame tile w of the 128-frame block.  M = 16 output channels,
//   N = 16 frames, K = 4 input channels per MFMA.
//   Operand mapping: MFMA step s (0 .. 3) of the 16-channel k block kb takes input channel 16 kb + 4 q + s from lane group q = lane >> 4.
//     B of step s = component s of the quad the lane holds for its own frame (channels 16 kb + 4 q .. + 3 of frame j): the layout of X, of
//       the ring quads and of the C / D fragment -- activations, residual stream and ring history go to the matrix pipe as they are;
//     A of the four steps = ONE 16-byte LDS read of the image [row block][k block][64 lanes] float4, lane (i = lane & 15, q) holding
//       W[16 rb + i][16 kb + 4 q .. + 3] -- the gather of the global load, committed as it is (1 KB per 16 x 16 block).
//   LDS: X[G][128] float4 (<= 64 KB) | head accumulator [G][128] up to 64 channels (in registers above: a lane only touches its own
//     (frame, group) positions) | the weight image(s) | the condition row.  A whole 128 x 128 matrix is 64 KB and fits beside X: no
//     sub-matrix passes.  Up to 96 channels two images fit and the next matrix is committed while the slower waves still read the
//     current one (one LDS-only barrier per mat-mul); at 128 channels there is one image, the next matrix waits in registers (8 float4
//     per thread) across the mat-mul and a second barrier frees the image before the commit.
//   One template over NB = 16-channel blocks per matrix side, instantiated for 2 / 4 / 6 / 8 (<= 32 / 64 / 96 / 128 channels): the
//     layer walk is the same at every width, what differs (where the head lives, one or two images, what is loaded ahead) is
//     constexpr in NB.  ONE instantiation per width whatever the stream count or block length.
//
// Sum order: acc[rb] += over kb ascending, s ascending, the MFMA's own four-way sum inside -- a function of the model alone, not of the
// frame's place in the block, the block length or the other streams: call sizes do not change a sample's bits.  The unit is compiled
// with -ffp-contract=off so that no instantiation fuses what another one rounds twice.
//
// Gated layer arrays (the A1 key "gated", WnPrewarmLayer::gated; loaded wider than 16 channels on request, NA_SetWaveNetWideGated):
// WaveNetWideF32Kernel<NB, true>, NB = 2 / 4 (<= 32 / 64 channels), compiled in a translation unit of their own
// (wavenet_wide_f32_gated_kernels.hip includes this file) so that the plain instantiations' code stays what it was.  A gated layer's
// conv, bias and mix-in have 2 C rows: rows 0 .. C-1 the filter half, C .. 2C-1 the gate half, z = act(filter) * sigmoid(gate).
//   One image per tap: the [2C x C] tap matrix as 2 nb x nb blocks -- filter rows in row blocks 0 .. nb-1, gate rows (from row C of the
//     file) in row blocks nb .. 2 nb-1, each half zero-padded to whole blocks on its own, so C = 17, 24, 33 .. need no special case.
//   The tap's B operands (the lane's quads of X or the ring) are fetched once and feed both halves; a lane's accumulator fragments
//     acc[rb] and accg[rb] hold the filter and gate pre-activations of the SAME four channels of the SAME frame: the gating is
//     lane-local -- no cross-lane move, no LDS.  MFMAs are issued in groups of two filter and two gate row blocks (four independent
//     accumulators, four LDS quads in registers at a time); per accumulator the sum order is the plain one, kb ascending, s ascending.
//   Epilogue: z = Activate(f + bc_f + wm_f cond) * sigmoid(g + bc_g + wm_g cond), the sigmoid 0.5 (FastTanh(0.5 g) + 1) or, under
//     StdMath, rcp(1 + exp2(-g log2 e)) -- the prewarm kernel's expressions.  1x1, residual, head accumulate, rechannel and head
//     stages are the plain ones; a plain array inside a gated model runs the plain layer body of the same instantiation (L.gated).
//   LDS at NB = 4: X 32 KB + head 32 KB + two 8 x 4-block images 2 x 32 KB + the condition row = 131 584 bytes: double-imaged.
//   Registers: 2 NB accumulator quads, b[] / zs[] stay NB, the staged matrix is 2 NB NB / 8 quads per thread; the bias / mix-in vectors
//     of both halves are loaded ahead like the plain ones at NB = 2, at use at NB = 4 (profiles/wide_gated_isa.txt: no scratch).
#include "device_once.h"

#include <hip/hip_runtime.h>

#include "wavenet_dev.h"
#include "wavenet_launch.h"

namespace na
{
	namespace wf
	{
		constexpr int FRAMES = WN_MAX_FRAMES;
		constexpr int NTHREADS = 512;
		typedef float f32x4 __attribute__((ext_vector_type(4)));
		typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4))); // a 16-byte load from a 4-byte aligned address

		// Activation.h:83-91
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

		// workgroup barrier that orders LDS traffic only: the weight loads of the next mat-mul (StageLoad) stay in flight across it.  (No
		// thread of the block reads global memory another one wrote in this launch: ring stores are history for LATER blocks.)
		__device__ __forceinline__ void LdsBarrier()
		{
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
			__builtin_amdgcn_s_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
		}

		// a row-major [cout x cin] matrix at w[off] (tap k of a layer conv at wconv is the matrix at wconv + k cout cin)
		struct MatRef
		{
			int off, cout, cin, nbo, nbk;
		};
		template <int NB>
		struct StagedRegs
		{
			static constexpr int ITEMS = (NB * NB * 64 + NTHREADS - 1) / NTHREADS;
			f32x4 v[ITEMS];
		};
		// image item idx = (block rb nbk + kb, lane (i, q)) <- W[16 rb + i][16 kb + 4 q .. + 3], zero outside the matrix
		template <int NB>
		__device__ __forceinline__ void StageLoad(StagedRegs<NB>& r, const float* __restrict__ w, const MatRef& m)
		{
#pragma unroll
			for (int it = 0; it < StagedRegs<NB>::ITEMS; it++)
			{
				const int idx = threadIdx.x + it * NTHREADS;
				const int lane = idx & 63, blk = idx >> 6, rb = blk / m.nbk, kb = blk % m.nbk;
				const int o = 16 * rb + (lane & 15), c0 = 16 * kb + 4 * (lane >> 4);
				const bool on = idx < m.nbo * m.nbk * 64 && o < m.cout;
				const float* p = w + m.off + (size_t)o * m.cin + c0;
				f32x4 v = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
				if (on && c0 + 3 < m.cin)
				{
					const f32x4u t = *reinterpret_cast<const f32x4u*>(p);
					v = f32x4{ t.x, t.y, t.z, t.w };
				}
				else if (on)
				{
					v.x = (c0 + 0 < m.cin) ? p[0] : 0.0f;
					v.y = (c0 + 1 < m.cin) ? p[1] : 0.0f;
					v.z = (c0 + 2 < m.cin) ? p[2] : 0.0f;
				}
				r.v[it] = v;
			}
		}
		template <int NB>
		__device__ __forceinline__ void StageCommit(f32x4* ops, const StagedRegs<NB>& r, const MatRef& m)
		{
#pragma unroll
			for (int it = 0; it < StagedRegs<NB>::ITEMS; it++)
			{
				const int idx = threadIdx.x + it * NTHREADS;
				if (idx < m.nbo * m.nbk * 64) ops[idx] = r.v[it];
			}
		}

		// The gated instantiations stage images of up to 2 NB x NB blocks (a gated layer's tap is [2C x C]).  gate: m describes ONE half ([cout x
		// cin] of the [2 cout x cin] matrix at m.off); the image then has 2 nbo row blocks, row block nbo + rb <- rows cout + 16 rb .. of the
		// matrix, each half zero-padded to whole blocks on its own.  !gate: the plain image of StageLoad.
		template <int NB>
		struct StagedRegsG
		{
			static constexpr int ITEMS = (2 * NB * NB * 64 + NTHREADS - 1) / NTHREADS;
			f32x4 v[ITEMS];
		};
		template <int NB>
		__device__ __forceinline__ void StageLoad(StagedRegsG<NB>& r, const float* __restrict__ w, const MatRef& m, bool gate = false)
		{
			const int half = m.nbo * m.nbk * 64;
#pragma unroll
			for (int it = 0; it < StagedRegsG<NB>::ITEMS; it++)
			{
				const int idx = threadIdx.x + it * NTHREADS;
				const bool g = gate && idx >= half;              // an item of the gate half
				const int idh = g ? idx - half : idx;
				const int lane = idh & 63, blk = idh >> 6, rb = blk / m.nbk, kb = blk % m.nbk;
				const int oh = 16 * rb + (lane & 15), c0 = 16 * kb + 4 * (lane >> 4);
				const bool on = idh < half && oh < m.cout;
				const float* p = w + m.off + (size_t)(g ? m.cout + oh : oh) * m.cin + c0;
				f32x4 v = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
				if (on && c0 + 3 < m.cin)
				{
					const f32x4u t = *reinterpret_cast<const f32x4u*>(p);
					v = f32x4{ t.x, t.y, t.z, t.w };
				}
				else if (on)
				{
					v.x = (c0 + 0 < m.cin) ? p[0] : 0.0f;
					v.y = (c0 + 1 < m.cin) ? p[1] : 0.0f;
					v.z = (c0 + 2 < m.cin) ? p[2] : 0.0f;
				}
				r.v[it] = v;
			}
		}
		template <int NB>
		__device__ __forceinline__ void StageCommit(f32x4* ops, const StagedRegsG<NB>& r, const MatRef& m, bool gate = false)
		{
#pragma unroll
			for (int it = 0; it < StagedRegsG<NB>::ITEMS; it++)
			{
				const int idx = threadIdx.x + it * NTHREADS;
				if (idx < (gate ? 2 : 1) * m.nbo * m.nbk * 64) ops[idx] = r.v[it];
			}
		}
		template <int NB, bool GATED>
		struct StagedOf
		{
			typedef StagedRegs<NB> T;
		};
		template <int NB>
		struct StagedOf<NB, true>
		{
			typedef StagedRegsG<NB> T;
		};

		// acc[rb] += M[16 rb .. + 16][all k blocks] * b[kb]   (b[kb] = the quad of channels 16 kb + 4 q .. of the lane's frame); k block by
		// k block, in groups of up to four row blocks: consecutive MFMAs write different accumulators, and a group's four LDS reads are all
		// of the image that is in registers at a time (the scheduling barrier keeps the compiler from hoisting the reads of the whole
		// unrolled mat-mul -- 64 quads at 128 channels -- in front of it; the SIMD's other wave covers the read latency)
		template <int NB>
		__device__ __forceinline__ void MatMul(const f32x4* ops, int nbo, int nbk, int lane, const f32x4 (&b)[NB], f32x4 (&acc)[NB])
		{
			constexpr int RH = NB < 4 ? NB : 4;
#pragma unroll
			for (int kb = 0; kb < NB; kb++)
			{
				if (kb >= nbk) break;
#pragma unroll
				for (int r0 = 0; r0 < NB; r0 += RH)
				{
					if (r0 >= nbo) break;
					f32x4 a[RH];
#pragma unroll
					for (int r = 0; r < RH; r++)
						if (r0 + r < NB && r0 + r < nbo) a[r] = ops[((r0 + r) * nbk + kb) * 64 + lane];
#pragma unroll
					for (int r = 0; r < RH; r++)
						if (r0 + r < NB && r0 + r < nbo) acc[(r0 + r) % NB] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].x, b[kb].x, acc[(r0 + r) % NB], 0, 0, 0);
#pragma unroll
					for (int r = 0; r < RH; r++)
						if (r0 + r < NB && r0 + r < nbo) acc[(r0 + r) % NB] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].y, b[kb].y, acc[(r0 + r) % NB], 0, 0, 0);
#pragma unroll
					for (int r = 0; r < RH; r++)
						if (r0 + r < NB && r0 + r < nbo) acc[(r0 + r) % NB] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].z, b[kb].z, acc[(r0 + r) % NB], 0, 0, 0);
#pragma unroll
					for (int r = 0; r < RH; r++)
						if (r0 + r < NB && r0 + r < nbo) acc[(r0 + r) % NB] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r].w, b[kb].w, acc[(r0 + r) % NB], 0, 0, 0);
					__builtin_amdgcn_sched_barrier(0);
				}
			}
		}

		// a gated tap: accf[rb] += F[16 rb .. + 16][.] * b, accg[rb] += G[16 rb .. + 16][.] * b from the image of 2 nb x nb blocks (StageLoad, gate) --
		// ONE set of B operands for both halves.  Groups of two filter and two gate row blocks: four independent accumulators behind each
		// other on the matrix pipe, four LDS quads in registers at a time.  Per accumulator: kb ascending, s ascending, as in MatMul.
		template <int NB>
		__device__ __forceinline__ void MatMulGated(const f32x4* ops, int nb, int lane, const f32x4 (&b)[NB], f32x4 (&accf)[NB], f32x4 (&accg)[NB])
		{
#pragma unroll
			for (int kb = 0; kb < NB; kb++)
			{
				if (kb >= nb) break;
#pragma unroll
				for (int r0 = 0; r0 < NB; r0 += 2)
				{
					if (r0 >= nb) break;
					const bool two = r0 + 1 < nb; // (NB is even; nb may be odd)
					const f32x4 f0 = ops[((r0)*nb + kb) * 64 + lane], g0 = ops[((nb + r0) * nb + kb) * 64 + lane];
					f32x4 f1 = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f }, g1 = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
					if (two)
					{
						f1 = ops[((r0 + 1) * nb + kb) * 64 + lane];
						g1 = ops[((nb + r0 + 1) * nb + kb) * 64 + lane];
					}
#define NA_WF_GATED_STEP(S)                                                                                   \
	accf[r0] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0.S, b[kb].S, accf[r0], 0, 0, 0);                        \
	accg[r0] = __builtin_amdgcn_mfma_f32_16x16x4f32(g0.S, b[kb].S, accg[r0], 0, 0, 0);                        \
	if (two)                                                                                                  \
	{                                                                                                         \
		accf[r0 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1.S, b[kb].S, accf[r0 + 1], 0, 0, 0);            \
		accg[r0 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(g1.S, b[kb].S, accg[r0 + 1], 0, 0, 0);            \
	}
					NA_WF_GATED_STEP(x)
					NA_WF_GATED_STEP(y)
					NA_WF_GATED_STEP(z)
					NA_WF_GATED_STEP(w)
#undef NA_WF_GATED_STEP
					__builtin_amdgcn_sched_barrier(0);
				}
			}
		}
		// Activation.h:40-43,93-96 -- the gate's sigmoid by the model's math policy (mode 2: StdMath), the prewarm kernel's expressions
		__device__ __forceinline__ float Sigmoid(float g, int mode)
		{
			if (mode == 2) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f));
			return 0.5f * (FastTanh(0.5f * g) + 1.0f);
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

		constexpr bool HeadInLds(int nb) { return nb <= 4; }   // up to 64 channels; in registers above
		constexpr bool TwoImages(int nb) { return nb <= 6; }   // X + two images within 160 KB (96 channels: 48 + 72 KB; 128: 64 + 128)
		constexpr bool LoadsAhead(int nb) { return nb <= 4; }  // bias vectors and the ring history of K <= 3 ahead of the taps (registers)
		constexpr size_t LdsBytes(int nb, int gq, bool gated = false)
		{
			return (size_t)(HeadInLds(nb) ? 2 : 1) * gq * FRAMES * 16 + (size_t)(TwoImages(nb) ? 2 : 1) * (gated ? 2 : 1) * nb * nb * 64 * 16 + FRAMES * sizeof(float);
		}

		template <int NB, bool GATED = false>
		__global__ void __launch_bounds__(NTHREADS) __attribute__((amdgpu_waves_per_eu(2))) WaveNetWideF32Kernel(const Args a, const float* __restrict__ in, float* __restrict__ out,
			long inStride, long outStride, int n)
		{
			static_assert(!GATED || NB <= 4, "gated: a [2C x C] tap is one image of at most 8 x 4 blocks");
			// (the gated <4> gives up the ahead loads -- bias vectors and ring history -- for its second accumulator set: with them it spills 25 VGPRs)
			constexpr bool HEAD_LDS = HeadInLds(NB), TWO = TwoImages(NB), AHEAD = LoadsAhead(NB) && !(GATED && NB > 2);
			constexpr bool AHEAD_G = GATED && AHEAD; // a gated layer's gate-half bias / mix-in vectors ahead as well
			constexpr int RB = GATED ? 2 * NB : NB;     // row blocks of the largest image
			constexpr int OPS_ONE = RB * NB * 64;
			extern __shared__ __attribute__((aligned(16))) float lds[];
			const int GQ = (a.maxC + 3) / 4;                          // channel groups of the widest array
			f32x4* X = reinterpret_cast<f32x4*>(lds);                 // [GQ][FRAMES]
			f32x4* HEAD = X + (size_t)GQ * FRAMES;                    // [GQ][FRAMES] (HEAD_LDS)
			f32x4* ops0 = HEAD + (HEAD_LDS ? (size_t)GQ * FRAMES : 0); // [TWO ? 2 : 1][RB * NB][64]
			float* condL = reinterpret_cast<float*>(ops0 + (TWO ? 2 : 1) * OPS_ONE); // [FRAMES]
			int par = 0; // mat-muls so far (workgroup-uniform)
			const int tid = threadIdx.x;
			const int f = tid & (FRAMES - 1), cq = tid >> 7;          // gather / ring role
			const int lane = tid & 63, wave = tid >> 6;               // mat-mul role: tile = wave
			const int j = lane & 15, q = lane >> 4, tf = 16 * wave + j; // the lane's frame
			const int sidx = blockIdx.x;
			const int slot = a.slots ? a.slots[sidx] : a.slot0 + sidx;
			const int row = a.slots ? a.rows[sidx] : a.row0 + sidx;
			float* st = a.state + (size_t)slot * (size_t)a.stateF4 * 4;
			f32x4* stq = reinterpret_cast<f32x4*>(st);
			int* header = reinterpret_cast<int*>(st);
			if (cq == 0) condL[f] = (f < n) ? in[(size_t)row * inStride + f] : 0.0f; // WaveNet.h:770 (input -> condition), as it is
			for (int g = cq; g < GQ; g += 4)
			{
				X[g * FRAMES + f] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
				if (HEAD_LDS) HEAD[g * FRAMES + f] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f }; // :772 headArray.SetZero()
			}
			f32x4 head[NB]; // !HEAD_LDS: the lane's head accumulator, group 4 rb + q of frame tf
#pragma unroll
			for (int rb = 0; rb < NB; rb++) head[rb] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
			__syncthreads();
			const float cond = condL[tf];

			const float* __restrict__ w = a.w;
			typename StagedOf<NB, GATED>::T pre;   // weights of the next mat-mul, under way while the current one runs
			bool havePre = false; // (workgroup-uniform)
			// the image the next mat-mul reads.  Two images: the one the mat-mul before the last read -- every wave is past that one (the
			// barrier in front of the last mat-mul).  One image: every wave must be past the LAST mat-mul first.
			auto nextImage = [&]() -> f32x4* {
				if (!TWO)
				{
					LdsBarrier();
					return ops0;
				}
				return ops0 + (par++ & 1) * OPS_ONE;
			};
			for (int li = 0; li < a.numLayers; li++)
			{
				const WnPrewarmLayer L = a.layers[li];
				if (L.kind == 0)
				{
					const int cin = L.cin; // == cout
					const int Gl = (cin + 3) / 4, nb = (cin + 15) / 16;
					const bool lg = GATED && L.gated != 0;                   // a gated layer (workgroup-uniform): taps of [2 cin x cin], two accumulator sets
					// AHEAD: the layer's bias / mix-in vectors for the rows this lane will hold, loaded now (they are used behind the mat-muls,
					// where a load is a memory round trip on the critical path); the widest instantiations need the registers and load at use
					f32x4 bcv[AHEAD ? NB : 1], wmv[AHEAD ? NB : 1], b1v[AHEAD ? NB : 1];
					if (AHEAD)
					{
#pragma unroll
						for (int rb = 0; rb < NB; rb++)
						{
							const int g = 4 * rb + q;
							const bool on = rb < nb && g < Gl;
							bcv[AHEAD ? rb : 0] = on ? Load4(w, L.bconv, 4 * g, cin) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
							wmv[AHEAD ? rb : 0] = on ? Load4(w, L.wmix, 4 * g, cin) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
							b1v[AHEAD ? rb : 0] = on ? Load4(w, L.b1, 4 * g, cin) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						}
					}
					// (gated layer: the gate half's bias and mix-in, rows cin .. 2 cin - 1 of both vectors)
					f32x4 bgv[AHEAD_G ? NB : 1], wgv[AHEAD_G ? NB : 1];
					if (AHEAD_G && lg)
					{
#pragma unroll
						for (int rb = 0; rb < NB; rb++)
						{
							const int g = 4 * rb + q;
							const bool on = rb < nb && g < Gl;
							bgv[AHEAD_G ? rb : 0] = on ? Load4(w, L.bconv + cin, 4 * g, cin) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
							wgv[AHEAD_G ? rb : 0] = on ? Load4(w, L.wmix + cin, 4 * g, cin) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						}
					}
					if (L.rechannel >= 0)
					{
						// rechannel (:637): array 0 from the condition (input_size == 1), later arrays from the previous array's output (in X)
						if (li == 0 && L.rech_in == 1)
						{
#pragma unroll
							for (int rb = 0; rb < NB; rb++)
							{
								const int g = 4 * rb + q;
								if (rb < nb && g < Gl) X[g * FRAMES + tf] = Load4(w, L.rechannel, 4 * g, cin) * cond;
							}
						}
						else
						{
							const int nbk = (L.rech_in + 15) / 16, Gin = (L.rech_in + 3) / 4;
							__syncthreads(); // the images are free (the previous array's head mat-mul is done everywhere)
							f32x4* ops = nextImage();
							const MatRef mr = { L.rechannel, cin, L.rech_in, nb, nbk };
							StageLoad<NB>(pre, w, mr);
							StageCommit<NB>(ops, pre, mr);
							f32x4 b[NB];
#pragma unroll
							for (int kb = 0; kb < NB; kb++)
								b[kb] = (kb < nbk && 4 * kb + q < Gin) ? X[(4 * kb + q) * FRAMES + tf] : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
							__syncthreads(); // image staged; every wave has read its own frames of the old X
							f32x4 acc[NB];
#pragma unroll
							for (int rb = 0; rb < NB; rb++) acc[rb] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
							MatMul<NB>(ops, nb, nbk, lane, b, acc);
#pragma unroll
							for (int rb = 0; rb < NB; rb++)
								if (rb < nb && 4 * rb + q < Gl) X[(4 * rb + q) * FRAMES + tf] = acc[rb];
						}
					}
					__syncthreads(); // X of every frame is complete; every wave is past the last mat-mul
					// the layer input of this block -> its ring (history for LATER blocks: only the last R - FRAMES frames can be read back)
					const int R = a.ringFrames[L.ring_id], G = a.ringG[L.ring_id], roff = a.ringOffF4[L.ring_id];
					const int pos0 = header[L.ring_id];
					{
						int p = pos0 + f;
						if (p >= R) p -= R;
						if (f < n && f >= n - (R - FRAMES))
							for (int g = cq; g < Gl; g += 4) stq[RingQuad(roff, G, p, g)] = X[g * FRAMES + f];
					}
					// dilated conv (:139-290), tap by tap: the tap's [cin x cin] matrix -> image, the tap's input where the mat-mul wants it (lane
					// = frame of the wave's tile, channel group 4 kb + q: X inside the block, the ring before it), accumulate on the matrix pipe
					const int K = L.ksize;
					f32x4 acc[NB];
#pragma unroll
					for (int rb = 0; rb < NB; rb++) acc[rb] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
					f32x4 accg[GATED ? NB : 1]; // gated layer: the gate half's pre-activations, the same channels and frame as acc[]
					if (GATED)
					{
#pragma unroll
						for (int rb = 0; rb < NB; rb++) accg[GATED ? rb : 0] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
					}
					auto histOf = [&](int k, f32x4 (&h)[NB]) {
						const int src = tf - L.dilation * (K - 1 - k);
						int p = pos0 + src; // src >= -(R - FRAMES): one wrap
						if (p < 0) p += R;
#pragma unroll
						for (int kb = 0; kb < NB; kb++)
						{
							const int g = 4 * kb + q;
							h[kb] = (src < 0 && kb < nb && g < Gl) ? stq[RingQuad(roff, G, p, g)] : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						}
					};
					auto tap = [&](int k, const f32x4 (&h)[NB]) {
						f32x4* ops = nextImage();
						if constexpr (GATED)
						{
							// the same with a gated layer's taps: [2 cin x cin] each in the tap-major copy, mk / mn describe the filter half
							const int tapFloats = lg ? 2 * cin * cin : cin * cin;
							const MatRef mk = { L.wconv + k * tapFloats, cin, cin, nb, nb };
							if (!havePre) StageLoad<NB>(pre, w, mk, lg);
							StageCommit<NB>(ops, pre, mk, lg);
							const MatRef mn = (k + 1 < K) ? MatRef{ L.wconv + (k + 1) * tapFloats, cin, cin, nb, nb } : MatRef{ L.w1, cin, cin, nb, nb };
							StageLoad<NB>(pre, w, mn, lg && k + 1 < K);
						}
						else
						{
							const MatRef mk = { L.wconv + k * cin * cin, cin, cin, nb, nb };
							if (!havePre) StageLoad<NB>(pre, w, mk); // (the first tap behind a rechannel / head stage: nothing was under way)
							StageCommit<NB>(ops, pre, mk);
							// the next mat-mul's weights set out now: the next tap's, or the 1x1's behind the last tap
							const MatRef mn = (k + 1 < K) ? MatRef{ L.wconv + (k + 1) * cin * cin, cin, cin, nb, nb } : MatRef{ L.w1, cin, cin, nb, nb };
							StageLoad<NB>(pre, w, mn);
						}
						havePre = true;
						LdsBarrier();
						const int src = tf - L.dilation * (K - 1 - k); // tap k reads the frame d (K-1-k) back
						f32x4 b[NB];
#pragma unroll
						for (int kb = 0; kb < NB; kb++)
						{
							const int g = 4 * kb + q;
							b[kb] = (kb < nb && g < Gl) ? (src >= 0 ? X[g * FRAMES + src] : h[kb]) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						}
						if constexpr (GATED)
						{
							if (lg) MatMulGated<NB>(ops, nb, lane, b, acc, accg);
							else MatMul<NB>(ops, nb, nb, lane, b, acc);
						}
						else MatMul<NB>(ops, nb, nb, lane, b, acc);
					};
					if (AHEAD && K <= 3)
					{
						// the ring part of up to three taps (every A1-shaped model) ahead of the whole tap loop: its HBM round trip runs behind
						// the first mat-muls
						f32x4 hist0[NB], hist1[NB], hist2[NB];
						histOf(0, hist0);
						if (K > 1) histOf(1, hist1);
						if (K > 2) histOf(2, hist2);
						tap(0, hist0);
						if (K > 1) tap(1, hist1);
						if (K > 2) tap(2, hist2);
					}
					else
					{
						f32x4 hist[NB];
						for (int k = 0; k < K; k++)
						{
							histOf(k, hist);
							tap(k, hist);
						}
					}
					// bias + mix-in (:288-289, :471), activation (:473-480), head accumulate (:482) -- in the lanes that hold the results; the
					// activation's quad IS the 1x1's B operand (result rows 16 rb + 4 q .. of the lane's frame = k block rb, group q)
					f32x4 zs[NB];
#pragma unroll
					for (int rb = 0; rb < NB; rb++)
					{
						zs[rb] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						const int g = 4 * rb + q;
						if (rb < nb && g < Gl)
						{
							const f32x4 bc = AHEAD ? bcv[AHEAD ? rb : 0] : Load4(w, L.bconv, 4 * g, cin);
							const f32x4 wm = AHEAD ? wmv[AHEAD ? rb : 0] : Load4(w, L.wmix, 4 * g, cin);
							f32x4 zv;
							zv.x = (4 * g + 0 < cin) ? Activate(acc[rb].x + bc.x + wm.x * cond, L.act) : 0.0f;
							zv.y = (4 * g + 1 < cin) ? Activate(acc[rb].y + bc.y + wm.y * cond, L.act) : 0.0f;
							zv.z = (4 * g + 2 < cin) ? Activate(acc[rb].z + bc.z + wm.z * cond, L.act) : 0.0f;
							zv.w = (4 * g + 3 < cin) ? Activate(acc[rb].w + bc.w + wm.w * cond, L.act) : 0.0f;
							if constexpr (GATED)
							{
								if (lg)
								{
									// z = act(filter) * sigmoid(gate): the gate's pre-activation is in this lane, same channels, same frame
									const f32x4 bg = AHEAD_G ? bgv[AHEAD_G ? rb : 0] : Load4(w, L.bconv + cin, 4 * g, cin);
									const f32x4 wg = AHEAD_G ? wgv[AHEAD_G ? rb : 0] : Load4(w, L.wmix + cin, 4 * g, cin);
									const f32x4 ag = accg[GATED ? rb : 0];
									if (4 * g + 0 < cin) zv.x *= Sigmoid(ag.x + bg.x + wg.x * cond, L.gated);
									if (4 * g + 1 < cin) zv.y *= Sigmoid(ag.y + bg.y + wg.y * cond, L.gated);
									if (4 * g + 2 < cin) zv.z *= Sigmoid(ag.z + bg.z + wg.z * cond, L.gated);
									if (4 * g + 3 < cin) zv.w *= Sigmoid(ag.w + bg.w + wg.w * cond, L.gated);
								}
							}
							if (HEAD_LDS) HEAD[g * FRAMES + tf] += zv;
							else head[rb] += zv;
							zs[rb] = zv;
						}
					}
					// 1x1 + bias + residual (:486-491); the last layer's output feeds the next array's rechannel (or nothing)
					f32x4* ops = nextImage();
					StageCommit<NB>(ops, pre, MatRef{ L.w1, cin, cin, nb, nb });
					havePre = false;
					if (li + 1 < a.numLayers)
					{
						// the first tap of the next layer, when nothing else is staged in between (same array: no rechannel, no head)
						const WnPrewarmLayer N = a.layers[li + 1];
						if (N.kind == 0 && N.rechannel < 0)
						{
							const int nbn = (N.cin + 15) / 16;
							if constexpr (GATED) StageLoad<NB>(pre, w, MatRef{ N.wconv, N.cin, N.cin, nbn, nbn }, N.gated != 0);
							else StageLoad<NB>(pre, w, MatRef{ N.wconv, N.cin, N.cin, nbn, nbn });
							havePre = true;
						}
					}
					LdsBarrier(); // image staged -- and every wave has read its taps' frames of X, which the residual changes
#pragma unroll
					for (int rb = 0; rb < NB; rb++) acc[rb] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
					MatMul<NB>(ops, nb, nb, lane, zs, acc);
#pragma unroll
					for (int rb = 0; rb < NB; rb++)
					{
						const int g = 4 * rb + q;
						if (rb < nb && g < Gl)
						{
							const f32x4 b1 = AHEAD ? b1v[AHEAD ? rb : 0] : Load4(w, L.b1, 4 * g, cin);
							X[g * FRAMES + tf] += f32x4{ acc[rb].x + b1.x, acc[rb].y + b1.y, acc[rb].z + b1.z, acc[rb].w + b1.w };
						}
					}
					// (the next stage starts with a barrier: X complete, images free)
				}
				else
				{
					// head rechannel (:658-660): becomes the next array's head accumulator (:785-789) or, for the last array, the output.
					// K = 1: a dense layer on the frame's own head column (matrix pipe).  K > 1 (a conv head, on the LAST array of up to 64
					// channels: ValidateWaveNetDesc): the head accumulator has its own ring -- publish, then every tap reads the frame
					// (K-1-k) head_dilation back, from LDS inside the block and from the ring before it (thread = frame, f32 VALU: the head has
					// few output channels).
					const bool last = (li == a.numLayers - 1);
					const int Gin = (L.cin + 3) / 4, nbk = (L.cin + 15) / 16, nbo = (L.cout + 15) / 16, Gout = (L.cout + 3) / 4;
					__syncthreads(); // HEAD of every frame is complete, every wave is past the last mat-mul
					if (L.ksize > 1)
					{
						// (a narrow last array behind one wider than 64 channels: the accumulator is in registers -- through the idle image:
						// Gin <= 16 groups x 2 KB within the 36 KB / 64 KB of one image of these instantiations)
						f32x4* HL = HEAD_LDS ? HEAD : ops0;
						if (!HEAD_LDS)
						{
#pragma unroll
							for (int rb = 0; rb < NB; rb++)
								if (rb < 4 && 4 * rb + q < Gin) HL[(4 * rb + q) * FRAMES + tf] = head[rb];
							__syncthreads();
						}
						const int R = a.ringFrames[L.ring_id], G = a.ringG[L.ring_id], roff = a.ringOffF4[L.ring_id];
						const int pos0 = header[L.ring_id];
						int p = pos0 + f;
						if (p >= R) p -= R;
						if (f < n && f >= n - (R - FRAMES))
							for (int g = cq; g < Gin; g += 4) stq[RingQuad(roff, G, p, g)] = HL[g * FRAMES + f];
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
									const f32x4 hv = (off >= 0) ? HL[g * FRAMES + off] : stq[RingQuad(roff, G, pq, g)];
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
						f32x4* ops = nextImage();
						const MatRef mh = { L.wconv, L.cout, L.cin, nbo, nbk };
						StageLoad<NB>(pre, w, mh);
						StageCommit<NB>(ops, pre, mh);
						f32x4 b[NB];
#pragma unroll
						for (int kb = 0; kb < NB; kb++)
						{
							const bool on = kb < nbk && 4 * kb + q < Gin;
							if (HEAD_LDS) b[kb] = on ? HEAD[(4 * kb + q) * FRAMES + tf] : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
							else b[kb] = on ? head[kb] : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						}
						__syncthreads();
						f32x4 acc[NB];
#pragma unroll
						for (int rb = 0; rb < NB; rb++) acc[rb] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
						MatMul<NB>(ops, nbo, nbk, lane, b, acc);
						if (last)
						{
							if (q == 0 && tf < n) out[(size_t)row * outStride + tf] = a.headScale * (acc[0].x + ((L.bconv >= 0) ? w[L.bconv] : 0.0f)); // :793-798
						}
						else
						{
#pragma unroll
							for (int rb = 0; rb < NB; rb++)
							{
								const int g = 4 * rb + q;
								if (g < GQ)
								{
									f32x4 v = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
									if (rb < nbo && g < Gout)
									{
										const f32x4 bb = (L.bconv >= 0) ? Load4(w, L.bconv, 4 * g, L.cout) : f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };
										v = f32x4{ acc[rb].x + bb.x, acc[rb].y + bb.y, acc[rb].z + bb.z, acc[rb].w + bb.w };
										if (4 * g + 1 >= L.cout) v.y = 0.0f;
										if (4 * g + 2 >= L.cout) v.z = 0.0f;
										if (4 * g + 3 >= L.cout) v.w = 0.0f;
									}
									if (HEAD_LDS) HEAD[g * FRAMES + tf] = v; // the lane owns (group, frame): read above, written here
									else head[rb] = v;
								}
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

		template <int NB, bool GATED = false>
		hipError_t Launch(const Args& a, int numStreams, const float* in, float* out, long inStride, long outStride, int n, hipStream_t stream)
		{
			static PerDeviceOnce attr;
			(void)attr.Run([] { return hipFuncSetAttribute(reinterpret_cast<const void*>(&WaveNetWideF32Kernel<NB, GATED>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
			hipLaunchKernelGGL((WaveNetWideF32Kernel<NB, GATED>), dim3((unsigned)numStreams), dim3(NTHREADS), LdsBytes(NB, (a.maxC + 3) / 4, GATED), stream, a, in, out, inStride, outStride, n);
			return hipGetLastError();
		}

		// the gated instantiations <2, true> / <4, true> (wavenet_wide_f32_gated_kernels.hip)
		hipError_t LaunchGated(const Args& a, int nb, int numStreams, const float* in, float* out, long inStride, long outStride, int n, hipStream_t stream);
#ifdef NA_WIDE_F32_GATED_TU
		// LDS at the widest model of each: 32 channels 49 664, 64: 131 584 bytes (of 163 840)
		hipError_t LaunchGated(const Args& a, int nb, int numStreams, const float* in, float* out, long inStride, long outStride, int n, hipStream_t stream)
		{
			if (nb == 2) return Launch<2, true>(a, numStreams, in, out, inStride, outStride, n, stream);
			if (nb == 4) return Launch<4, true>(a, numStreams, in, out, inStride, outStride, n, stream);
			return hipErrorInvalidValue;
		}
#endif
	}

#ifndef NA_WIDE_F32_GATED_TU
	hipError_t LaunchWaveNetWideF32(const WnPrewarmLayer* layers, int numLayers, const float* weights, const int* ringOffF4, const int* ringFrames, const int* ringG,
		int nrings, int stateF4, int maxChannels, float headScale, bool gated, float* state, const int* slots, const int* rows, int numStreams, int slot0, int row0,
		const float* in, float* out, long inStride, long outStride, int n, hipStream_t stream)
	{
		if (numStreams <= 0 || n <= 0) return hipSuccess;
		const WaveNetWideF32Choice c = WaveNetWideF32For(maxChannels, gated); // (nb == 0: no instantiation -- beyond 128 channels, gated beyond 64)
		if (n > WN_MAX_FRAMES || c.nb == 0) return hipErrorInvalidValue;
		wf::Args a;
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
		if (c.gated) return wf::LaunchGated(a, c.nb, numStreams, in, out, inStride, outStride, n, stream);
		// LDS at the widest model of each instantiation: 32 channels 41 472, 64: 98 816, 96: 123 392, 128: 131 584 bytes (of 163 840)
		if (c.nb == 2) return wf::Launch<2>(a, numStreams, in, out, inStride, outStride, n, stream);
		if (c.nb == 4) return wf::Launch<4>(a, numStreams, in, out, inStride, outStride, n, stream);
		if (c.nb == 6) return wf::Launch<6>(a, numStreams, in, out, inStride, outStride, n, stream);
		return wf::Launch<8>(a, numStreams, in, out, inStride, outStride, n, stream);
	}
#endif
}
