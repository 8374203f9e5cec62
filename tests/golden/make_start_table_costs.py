"""Records tests/golden/start_table_wave_costs.npz: the sr_wave_costs maps
(per 8x8 wave: the longest ray's steps and the wave's budget events) that
tests/test_gpu_start_table.py::test_same_budgets_as_before holds the kernel
to. The fixture is the record of the commit BEFORE the start table, so run
this against a library built from that commit (needs a HIP device):

    git worktree add /tmp/parent <commit before the start table>
    make -C /tmp/parent/schwarzschild-raytracer_amd
    SR_LIB=/tmp/parent/schwarzschild-raytracer_amd/lib/libsr.so python tests/golden/make_start_table_costs.py

The cases (scenes, cameras, overlay, size, steps) are the test's own
wave_cost_maps.
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
    import test_gpu_start_table as T

    out = Path(sys.argv[1]) if len(sys.argv) > 1 else T.COSTS
    pkg, oracle = srpkg.load_package(), srpkg.load_oracle()
    golden = np.load(ROOT / "tests" / "golden" / "golden.npz")
    h, w = (int(v) for v in golden["meta_skybox_shape"])  # conftest's textures fixture
    textures = (pkg.scenes.skybox(w, h), pkg.scenes.default_texture_array()[0])
    wd = T.start_world(pkg, oracle, textures)
    gpu = T.new_renderer(pkg, textures)
    maps = T.wave_cost_maps(gpu, wd)
    again = T.wave_cost_maps(gpu, wd)
    gpu.close()
    assert all(np.array_equal(maps[k], again[k]) for k in maps), "two recordings differ"
    np.savez_compressed(out, **maps)
    events = sum(int(a[..., 1].sum()) for a in maps.values())
    print(f"{out}: {len(maps)} maps, {events} budget events, library {os.environ.get('SR_LIB', 'lib/libsr.so')}")


if __name__ == "__main__":
    main()
