"""Writes the parent figures of tests/test_gpu_small_kernel_floors.py: every case of that test measured (max error against its float64
reference, SHA-256 of the output bytes) with the library that DPMN_HIP_LIB names -- a build of the PARENT commit's csrc:

    DPMN_HIP_LIB=/path/to/parent/libdpmn_hip.so python tools/record_small_kernel_floors.py profiles/r16a_small_kernel_floors_parent.json

Run once per change of those kernels, on the GPU; the test then holds the new kernels to twice these errors and to these bits.
Shapes, inputs and the float64 reference are the test module's own, so that both sides measure the same thing; what keeps a shared mistake
from hiding is that the reference is plain torch on the CPU (F.conv2d, F.layer_norm, F.gelu, softmax) and that the error bound is absolute evidence on
its own: a parent error far above fp32 round-off in the JSON would show it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(out_path):
    import torch
    import test_gpu_small_kernel_floors as t
    assert os.environ.get("DPMN_HIP_LIB"), "name the parent build in DPMN_HIP_LIB"
    dev = torch.device("cuda:0")
    cases = {}
    for shape in t.DW_SHAPES + t.DW_STREAM_SHAPES:
        cases.update(t.dw_measure(dev, *shape))
    for shape in t.SK_SHAPES:
        cases.update(t.sk_measure(dev, *shape))
    for shape in t.PE_SHAPES:
        cases.update(t.pe_measure(dev, *shape))
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"what": "parent-kernel figures of tests/test_gpu_small_kernel_floors.py (tools/record_small_kernel_floors.py)",
                   "library": "a build of the parent commit's dpmn_amd/csrc (DPMN_HIP_LIB)",
                   "device": torch.cuda.get_device_name(0), "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(cases), out_path))


if __name__ == "__main__":
    main(sys.argv[1])
