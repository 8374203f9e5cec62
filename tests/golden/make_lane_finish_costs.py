"""Records tests/golden/lane_finish_wave_costs.npz: the sr_wave_costs maps
(per 8x8 wave: the longest ray's steps and the wave's budget events) that
tests/test_gpu_lane_finish.py::test_wave_costs_as_before holds the kernel to.
The fixture is the record of the commit BEFORE parked lanes were finished
once per loop exit, so run this against a library built from that commit
(needs a HIP device):

    SR_LIB=<the parent's lib/libsr.so> python tests/golden/make_lane_finish_costs.py [out.npz]

The cells (scenes, cameras, steps, u_f, revolutions) are the test's own COST_CELLS.
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    import srpkg
    import test_gpu_lane_finish as T

    out = Path(sys.argv[1]) if len(sys.argv) > 1 else T.COSTS
    pkg, oracle = srpkg.load_package(), srpkg.load_oracle()
    golden = np.load(ROOT / "tests" / "golden" / "golden.npz")
    h, w = (int(v) for v in golden["meta_skybox_shape"])  # conftest's textures fixture
    textures = (pkg.scenes.skybox(w, h), pkg.scenes.default_texture_array()[0])
    wd = T.Cells(pkg, oracle, textures)
    gpu = pkg.Renderer(0)
    gpu.set_background(textures[0])
    gpu.set_texture_array(textures[1])
    maps = T.wave_cost_maps(gpu, wd)
    again = T.wave_cost_maps(gpu, wd)
    gpu.close()
    assert all(np.array_equal(maps[k], again[k]) for k in maps), "two recordings differ"
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(out, **maps)
    events = sum(int(a[..., 1].sum()) for a in maps.values())
    print(f"{out}: {len(maps)} maps, {events} budget events, library {os.environ.get('SR_LIB', 'lib/libsr.so')}")


if __name__ == "__main__":
    main()
