"""VoxelGrid off the easy path in the CPU tier: the `-m gpu` cases of tests/test_gpu_voxelgrid_regimes.py run on the wavefront
emulation of tests/wavesim (the recipe of tests/test_cluster_wavesim.py: PCLHIP_LIB = the emulation, PCLHIP_ALLOW_WAVESIM=1,
in a subprocess), all but the device-tensor case (`torch`) and the case that sizes itself from the device's CU count
(`fullgrid`).  With its 16 CUs the emulation takes the row kernel's second round and the key kernel's second trip at 4,133
voxels of 9 points already; no case takes more than a few seconds there."""
from test_cluster_wavesim import on_the_emulation, wavesim_lib  # noqa: F401  (the fixture that builds the emulation)


def test_voxelgrid_regimes_on_the_emulation(wavesim_lib):  # noqa: F811
    on_the_emulation(wavesim_lib, "test_gpu_voxelgrid_regimes.py", "not torch and not fullgrid")
