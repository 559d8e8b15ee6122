// recurrent_launch.cpp -- one block of a recurrent model on the kernel that RecurrentKernelFor chose for it (lstm_dev.h): a switch.
// The policy is in lstm_dev.h, the kernels and their launchers in lstm_kernels.hip / gru_kernels.hip / recurrent_dpp_kernels.hip.
#include <hip/hip_runtime_api.h>

#include "lstm_launch.h"

namespace na
{
	hipError_t LaunchRecurrentBlock(const RecurrentChoice& choice, const RecurrentBlock& b)
	{
		if (b.numStreams <= 0 || b.n <= 0) return hipSuccess;
		if (b.n > LSTM_MAX_FRAMES) return hipErrorInvalidValue;
		switch (choice.kernel)
		{
		case RecurrentKernel::Dpp:
		{
			const RecurrentGroup g = { b.m, b.state, b.capacity, b.slots, b.rows, b.numStreams };
			return LaunchRecurrentDpp(&g, 1, b.in, b.out, b.inStride, b.outStride, b.n, b.stream);
		}
		case RecurrentKernel::LstmWave: return LaunchLstmWave(b);
		case RecurrentKernel::GruWave: return LaunchGruWave(b);
		case RecurrentKernel::WaveRt: return LaunchRecurrentWaveRt(choice.plan, b);
		case RecurrentKernel::LstmBlock: return LaunchLstmBlockH(b);
		case RecurrentKernel::LstmGeneric: return LaunchLstmGeneric(b);
		case RecurrentKernel::GruGeneric: return LaunchGruGeneric(b);
		case RecurrentKernel::None: break;
		}
		// No kernel takes the shape under the process's tuning knobs.  Nothing is decided here any more: what follows only keeps the error
		// codes of the launchers this replaced (hipErrorNotSupported for a tail with conv1d layers that the runtime-shaped kernel cannot
		// take, except for a GRU shape that LaunchGruBlock refused with hipErrorInvalidValue before it looked at the tail)
		const LstmModelDev& m = b.m;
		const bool convTail = m.tailLayers > 0 && m.tailHistMax > 0;
		return (convTail && (m.cell != LSTM_CELL_GRU || GruShapeSupported(m.hidden, m.numLayers, m.tailWidth, m.tailHistMax))) ? hipErrorNotSupported : hipErrorInvalidValue;
	}
}
