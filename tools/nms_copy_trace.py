"""Three rotated-NMS calls at N = 16 384 through sst_amd.nms_gpu, then three through the iou3d_cuda shim (whose contract
copies the keep list to a CPU tensor), for a memory-copy trace:

    rocprofv3 --memory-copy-trace --stats --output-format csv -d DIR -o nms -- python tools/nms_copy_trace.py

The [N, ceil(N / 64)] mask is 33.5 MB; the keep list of the shim calls is ~94 KB per call.  Copies of a few KB (the
kept count, the score upload) are done by the runtime without a copy record and do not show in such a trace."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sst_amd import box_ops as B  # noqa: E402
from sst_amd import native_shims as S  # noqa: E402

g = torch.Generator().manual_seed(0)
n = 16384
c = (torch.rand(n, 2, generator=g) * 2 - 1) * 153.6
s = torch.rand(n, 2, generator=g) * 4 + 0.8
boxes = torch.cat([c - s / 2, c + s / 2, (torch.rand(n, 1, generator=g) * 2 - 1) * 3.14], 1).cuda()
scores = torch.rand(n, generator=g).cuda()
torch.cuda.synchronize()
for _ in range(3):
    keep = B.nms_gpu(boxes, scores, 0.25)
torch.cuda.synchronize()
order = scores.sort(0, descending=True)[1]
sorted_boxes = boxes[order].contiguous()
for _ in range(3):
    keep_cpu = torch.zeros(n, dtype=torch.long)
    num = S.iou3d_cuda.nms_gpu(sorted_boxes, keep_cpu, 0.25, 0)
torch.cuda.synchronize()
print(f'kept {keep.numel()} (shim {num}); mask bytes {n * ((n + 63) // 64) * 8}; keep-list bytes {num * 8}')
