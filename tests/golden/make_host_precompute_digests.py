#!/usr/bin/env python3
"""Records tests/golden/host_precompute_digests.json: SHA-256 digests of what
the host precomputation yields for the cases of tests/host_precompute_cases.py
(the scene image and segment buffer sr_set_scene + sr_set_test_ray upload, the
frame struct a whole-frame sr_render builds, the opacity bitmap).

The digests are a record of the code BEFORE that arithmetic moved into
csrc/host/precompute.cpp, not of the code under test. They were made from a
checkout of commit bcdebd6 ("Add equirectangular and fisheye projections to
every launch path"), whose sr_api.cpp still held the arithmetic inline, with
only these additions: the sr_debug_pack_scene / sr_debug_frame /
sr_debug_opacity_bits exports, which there ran that revision's own unmoved
sr_set_scene, sr_set_test_ray, launch() and make_opacity_map on a context
without a device (the HIP calls skipped, the buffers they would have uploaded
kept), plus this script, tests/host_precompute_cases.py and the abi.py
bindings of the exports. Run there as

    python tests/golden/make_host_precompute_digests.py

and the JSON was copied here unchanged. Running it on a later revision
records that revision's own output: only do that for a deliberate change of
the packed bytes, and say so in the commit.

The scene, frame and test-ray digests go through the C library's sqrt / cos /
acos in binary64 (glibc's, correctly rounded in practice); the step table is
not recorded here, tests/test_host_precompute.py checks it against a
restatement instead.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import srpkg  # noqa: E402


def main() -> None:
    import host_precompute_cases as cases

    pkg = srpkg.load_package()
    out = cases.compute(pkg)
    path = ROOT / "tests" / "golden" / "host_precompute_digests.json"
    path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(path, {k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
