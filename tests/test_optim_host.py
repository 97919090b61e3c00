"""CPU-side checks of the native optimizer step (csrc/optim.hip, hirest_amd/optim.py): the entry points exist and refuse bad
arguments before any launch, the chunk map covers every element once, the host derives AdamW's scalars as torch does, the
constructor refuses what the kernels do not implement, and the kernels neither spill nor use scratch memory."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _items(count, **over):
    from hirest_amd._lib import OptimItem
    arr = (OptimItem * count)()
    X = 1 << 20                    # placeholder addresses: every call below is refused by its argument checks, none is dereferenced
    for i, it in enumerate(arr):
        it.p, it.g, it.m, it.v, it.n = X, X, X, X, 100 + i
        for k, v in over.items():
            setattr(it, k, v)
    return arr


def test_entry_points_refuse_bad_arguments_without_gpu(lib):
    from hirest_amd._lib import OptimItem, OPTIM_GROUP_MAX, OPTIM_CHUNK
    hdr = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    assert f"#define HIREST_OPTIM_GROUP_MAX {OPTIM_GROUP_MAX}\n" in hdr and f"#define HIREST_OPTIM_CHUNK {OPTIM_CHUNK}\n" in hdr
    # hirest_optim_item: four pointers and an int64 count
    assert ctypes.sizeof(OptimItem) == 40 and OptimItem.n.offset == 32 and OptimItem.g.offset == 8
    BAD, X = -1, 1 << 20
    hp = (0.99, 0.1, 0.999, 0.001, 1e-3, 0.03, 1e-8)
    ok, big = _items(3), _items(OPTIM_GROUP_MAX + 1)
    for items, count in ((None, 3), (ok, 0), (ok, -1), (big, OPTIM_GROUP_MAX + 1)):
        assert lib.hirest_optim_partials_count(items, count) == BAD
        assert lib.hirest_grad_sqnorm_grouped_f32(items, count, X, None) == BAD
        assert lib.hirest_adamw_grouped_f32(items, count, None, *hp, None) == BAD
    assert lib.hirest_grad_sqnorm_grouped_f32(ok, 3, None, None) == BAD                    # no partials array
    for field in ("p", "g", "m", "v"):                                                     # a NULL tensor, a non-positive length
        assert lib.hirest_adamw_grouped_f32(_items(2, **{field: None}), 2, None, *hp, None) == BAD
    assert lib.hirest_adamw_grouped_f32(_items(2, n=0), 2, None, *hp, None) == BAD
    assert lib.hirest_grad_sqnorm_grouped_f32(_items(2, g=None), 2, X, None) == BAD
    assert lib.hirest_grad_sqnorm_grouped_f32(_items(2, n=-5), 2, X, None) == BAD
    assert lib.hirest_adamw_grouped_f32(ok, 3, None, 0.99, 0.1, 0.999, 0.001, 1e-3, 0.0, 1e-8, None) == BAD    # sqrt(bc2) = 0: step 0
    assert lib.hirest_clip_coef_f32(None, 4, 1.0, X, None) == BAD
    assert lib.hirest_clip_coef_f32(X, 4, 1.0, None, None) == BAD
    assert lib.hirest_clip_coef_f32(X, 0, 1.0, X, None) == BAD
    # more chunks than a grid has workgroups
    assert lib.hirest_optim_partials_count(_items(2, n=OPTIM_CHUNK << 31), 2) == -2
    assert lib.hirest_adamw_grouped_f32(_items(2, n=OPTIM_CHUNK << 31), 2, None, *hp, None) == -2


SIZE_LISTS = lambda c: [[1], [3, 64, 65], [c - 1, c, c + 1, 2 * c + 7], [5] * 150 + [c + 1] * 3]


def test_chunk_map_covers_every_element_once(lib):
    from hirest_amd import optim
    from hirest_amd._lib import OptimItem, OPTIM_GROUP_MAX
    c = optim.OPTIM_CHUNK
    for sizes in SIZE_LISTS(c):
        cm = optim.chunk_map(sizes)
        assert cm == optim.chunk_map(list(sizes))                 # a pure function of the sizes
        seen = [bytearray(n) for n in sizes]
        for item, start, count in cm:
            assert 0 < count <= c and start % c == 0 and start + count <= sizes[item]       # inside ONE tensor
            for e in range(start, start + count):
                seen[item][e] += 1
        assert all(all(b == 1 for b in s) for s in seen)
        assert [i for i, _, _ in cm] == sorted(i for i, _, _ in cm)                          # workgroup order = item order, then offset
        # launches of at most HIREST_OPTIM_GROUP_MAX items; the library counts the same chunks per launch
        ranges = optim.group_ranges(len(sizes))
        assert ranges[0][0] == 0 and ranges[-1][1] == len(sizes) and all(0 < hi - lo <= OPTIM_GROUP_MAX for lo, hi in ranges)
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        for lo, hi in ranges:
            arr = (OptimItem * (hi - lo))()
            for it, n in zip(arr, sizes[lo:hi]):
                it.g, it.n = 1 << 20, n
            assert lib.hirest_optim_partials_count(arr, hi - lo) == sum(1 for i, _, _ in cm if lo <= i < hi)
    assert len(optim.group_ranges(153)) == 3
    with pytest.raises(ValueError):
        optim.chunk_map([4, 0])


def test_hyperparameters_match_torch_double_expressions():
    from hirest_amd import optim
    lr, (b1, b2), eps, wd = 3e-4, (0.9, 0.999), 1e-8, 0.01
    for step in (1, 2, 1000):
        h = optim.hyperparameters(step, lr, (b1, b2), eps, wd)
        t = float(torch.tensor(float(step), dtype=torch.float32).item())       # torch's _get_value(step_t)
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t                                    # torch/optim/adam.py, the default (non-capturable) path
        assert h["bc1"] == bc1 and h["bc2_sqrt"] == bc2 ** 0.5 and h["step_size"] == lr / bc1
        assert h["decay"] == 1 - lr * wd and h["one_minus_beta1"] == 1 - b1 and h["one_minus_beta2"] == 1 - b2 and h["beta2"] == b2


def test_constructor_refusals():
    from hirest_amd import optim
    with pytest.raises(ValueError):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4))])                                   # CPU parameter
    with pytest.raises(ValueError):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16, device="meta"))])   # not fp32, whatever the device
    with pytest.raises(ValueError):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, device="meta"))], amsgrad=True)
    with pytest.raises(ValueError):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, device="meta"))], maximize=True)
    import hirest_amd
    assert hirest_amd.optim.AdamW is optim.AdamW and issubclass(optim.AdamW, torch.optim.Optimizer)


def _kernel_notes(obj_path, tmp_path):
    """{kernel symbol: its counters} from the AMDGPU metadata notes of the gfx950 code object inside one hipcc object."""
    llvm = "/opt/rocm/lib/llvm/bin"
    tool = lambda n: os.path.join(llvm, n) if os.path.isfile(os.path.join(llvm, n)) else shutil.which(n)
    objcopy, bundler, readelf = (tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"))
    if not all((objcopy, bundler, readelf)):
        pytest.skip("LLVM binutils of the ROCm toolchain not found")
    fat, co = os.path.join(tmp_path, "optim.fatbin"), os.path.join(tmp_path, "optim.co")
    subprocess.check_call([objcopy, "-O", "binary", "--only-section=.hip_fatbin", obj_path, fat])
    subprocess.check_call([bundler, "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    out, cur = {}, None
    for line in subprocess.check_output([readelf, "--notes", co], text=True).splitlines():
        m = re.match(r"\s+\.(name|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\S+)", line)
        if m and m.group(1) == "name":
            cur = out.setdefault(m.group(2), {})
        elif m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return {k: v for k, v in out.items() if "vgpr_count" in v}       # (argument records carry .name too, but no counters)


def test_optim_kernels_do_not_spill(lib, tmp_path):
    """Streaming kernels at 8 waves per SIMD: no spilled register, no scratch memory (the item table is indexed in the kernel
    arguments, not copied to private memory).  Read from the AMDGPU metadata notes as tests/test_code_objects.py does."""
    notes = _kernel_notes(os.path.join(REPO, "hirest_amd", "lib", "optim.o"), str(tmp_path))
    assert len(notes) == 3 and all(any(k in name for name in notes) for k in ("grad_sqnorm_kernel", "clip_coef_kernel", "adamw_kernel")), sorted(notes)
    for k, v in notes.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 64, (k, v)                      # 8 waves per SIMD
