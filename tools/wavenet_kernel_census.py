#!/usr/bin/env python3
"""Which kernels the WaveNet models launch: tools/wavenet_kernel_census.py  (run under `rocprofv3 --kernel-trace -- python ...`).

Processes ONE buffer each of a fixed list of batches, in that order, without prewarm; the first batch of every family also at the block
lengths 64, 32, 48 and 16.  With no knob set it reaches, of the launch decision (csrc/wavenet_launch_choice.h WaveNetLaunchFor): the chains
of the Standard, lite (padded and packed) and A2 families at 128 / 64 / 32 frames with half-size workgroups (SPB 1), the table launch, the
stage interpreter at two tiles per wave plain / generic / packed with 1, 2 and 4 waves per stream, the frame kernel at both block sizes and
the runtime-shaped kernel.  It does NOT reach the full-size workgroups (600 Standard streams run as two half batches of 300), the
non-temporal chains, the interpreter at four tiles per wave, or the one-tile chain (Nano packs dense to 16 / 8 by default; NA_WN_DENSE=0
makes it 16 / 16 and the small Nano batch then runs FamLite16T1): tests/test_wavenet_dispatch_cpu.py covers those branches on the CPU.
The ordered list of dispatched kernel names (with template arguments) in the trace is the census: two builds of the library launch the same kernels if their lists are equal (NA_LIB_SUFFIX selects a build under tools/variants/).
Tuning knobs (NA_WN_SPEC=0, NA_SP_SPB=1, NA_FR_PF=2 ...) move launches between instantiations; the printed lines say what
NA_BatchStreamKernelName answers for the first stream of each batch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np
import neuralaudio_amd as na
import na_oracle as O
import frame_cases as FC
import split_cases as SC
import wide_cases as WC

loader = na.NeuralModelLoader()


def from_file(name):
    return loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False)


def from_arrays(arrays, w):
    return loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam", doPrewarm=False)


lite = loader.CreateFromString(O.nam_json_wavenet_a1(12, 6, O.synth_wavenet_weights(O.a1_arrays(12, 6), seed=3)), ".nam", doPrewarm=False)
plain = SC.plain_custom()
plain = from_arrays(plain["arrays"], SC.weights(plain))
k2 = FC.small_k2_model()
k2 = from_arrays(k2["arrays"], FC.weights(k2))
wide = WC.chain([32], [([3, 3], [1, 64])])
wide = from_arrays(wide, O.synth_wavenet_weights(wide, seed=32))
std, feather, nano, a2 = (from_file("BossWN-%s.nam" % n) for n in ("standard", "feather", "nano", "a2"))
ALL_BLOCKS = (128, 64, 32, 48, 16)
# (name, [(model, streams, quality)], block lengths)
BATCHES = [("standard x 3", [(std, 3, 1.0)], ALL_BLOCKS), ("standard x 600", [(std, 600, 1.0)], (128,)),
           ("lite (padded) x 3", [(lite, 3, 1.0)], ALL_BLOCKS), ("feather (packed) x 6", [(feather, 6, 1.0)], ALL_BLOCKS),
           ("nano (packed) x 8", [(nano, 8, 1.0)], ALL_BLOCKS), ("nano (packed) x 1100", [(nano, 1100, 1.0)], (128,)),
           ("lite + feather + nano, 3 + 4 + 8", [(lite, 3, 1.0), (feather, 4, 1.0), (nano, 8, 1.0)], (128,)),
           ("a2 full x 3", [(a2, 3, 1.0)], ALL_BLOCKS), ("a2 lite x 3", [(a2, 3, 0.0)], (128,)),
           ("custom 16 / 8 x 3", [(plain, 3, 1.0)], ALL_BLOCKS), ("custom 16 / 8 x 3 beside a2 full x 3", [(plain, 3, 1.0), (a2, 3, 1.0)], (128,)),
           ("frame model 8 channels, K = 2, x 3", [(k2, 3, 1.0)], ALL_BLOCKS), ("32 channels x 3", [(wide, 3, 1.0)], ALL_BLOCKS),
           ("nine standard-shaped models x 1", [(from_file("BossWN-standard.nam"), 1, 1.0) for _ in range(9)], (128,))]

for name, members, blocks in BATCHES:
    b = na.Batch(0)
    for model, streams, quality in members:
        b.AddStreams(model, streams, quality, doPrewarm=False)
    for n in blocks:
        x = np.stack([O.signal_noise(n, 5 + s % 7) for s in range(b.NumStreams())])
        try:
            y = b.Process(x)
            print("%-40s n %3d  %-22s finite %s" % (name, n, b.StreamKernelName(0), bool(np.isfinite(y).all())), flush=True)
        except na.NeuralAudioError as e:  # (a knob that leaves the launch without a kernel: it is refused, the census goes on)
            print("%-40s n %3d  no kernel: %s" % (name, n, e), flush=True)
    b.close()
