"""Generates tests/golden/workspace_layout.json (tests/workspace_layout_util.py says what it holds) from the library as it is built NOW: run it
on the commit whose layout is to be pinned.  Without arguments: the "emul" table, through the CPU emulator (which reports one CU).  With
--gpu: the "gpu" table, through librtfe.so on the device, stored with the device's CU count (the deferred candidates' capacity depends on it).
The other table of an existing file is kept."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import workspace_layout_util as wl  # noqa: E402
from readtape_amd import frontend  # noqa: E402


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else wl.GOLDEN
    doc = wl.load_golden() if os.path.exists(wl.GOLDEN) else {}
    doc["row_counts"] = wl.ROW_COUNTS
    if "--gpu" in sys.argv:
        import torch
        doc["gpu"] = dict(num_cus=int(torch.cuda.get_device_properties(0).multi_processor_count), table=wl.build_table(frontend.FrontEnd))
    else:
        from emul_util import NumpyBackend, build_emul
        doc["emul"] = dict(num_cus=1, table=wl.build_table(lambda cfg: frontend.FrontEnd(cfg, _lib_path=build_emul(), _backend=NumpyBackend())))
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(out, {k: len(v["table"]) for k, v in doc.items() if isinstance(v, dict)}, "handles x", len(wl.ROW_COUNTS), "row counts")


if __name__ == "__main__":
    main()
