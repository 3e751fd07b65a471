"""CPU: every device kernel of libgsdr.so lives in exactly one code object -- the one of the translation unit whose
host code can launch it. A launcher that instantiates kernels in a header every unit includes puts dead copies
of them into each unit's code object (device code is emitted whether or not the unit has a host stub for it).
Reads symbol names only."""
import glob
import os
import struct
import subprocess
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"  # 24 bytes
COMPRESSED_MAGIC = b"CCOB"


def code_objects(lib_path, workdir):
    """The amdgcn code objects of the library's .hip_fatbin section, one bytes object per bundle entry."""
    fatbin = os.path.join(workdir, "fatbin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib_path, fatbin], check=True)
    assert os.path.exists(fatbin) and os.path.getsize(fatbin) > 0, "no .hip_fatbin section"
    data = open(fatbin, "rb").read()
    assert not data.startswith(COMPRESSED_MAGIC), "compressed offload bundles: nothing to read symbols from"
    assert data.startswith(BUNDLE_MAGIC), "the section does not start with an offload bundle"
    objs = []
    at = data.find(BUNDLE_MAGIC)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", data, at + len(BUNDLE_MAGIC))
        pos = at + len(BUNDLE_MAGIC) + 8
        for _ in range(count):
            offset, size, idlen = struct.unpack_from("<QQQ", data, pos)
            ident = data[pos + 24:pos + 24 + idlen].decode()
            pos += 24 + idlen
            if "amdgcn" in ident:
                assert size > 0 and at + offset + size <= len(data), ident
                objs.append(data[at + offset:at + offset + size])
        at = data.find(BUNDLE_MAGIC, at + 1)
    return objs


def kernels_of(obj, workdir):
    """Kernel names of one code object: its kernel descriptors are the symbols `<name>.kd`."""
    path = os.path.join(workdir, "code_object")
    with open(path, "wb") as f:
        f.write(obj)
    out = subprocess.run(["nm", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1][:-3] for line in out.splitlines() if line.endswith(".kd")]


def test_no_kernel_in_two_code_objects(tmp_path):
    from gsdr_amd import abi

    objs = code_objects(abi.LIB_PATH, str(tmp_path))
    units = glob.glob(os.path.join(ROOT, "gsdr_amd", "csrc", "*.hip"))
    assert len(objs) == len(units) > 0  # one code object per translation unit
    names = Counter()
    for obj in objs:
        kernels = kernels_of(obj, str(tmp_path))
        assert len(kernels) > 0
        assert len(set(kernels)) == len(kernels)
        names.update(kernels)
    total, distinct = sum(names.values()), len(names)
    print(f"{len(objs)} code objects, {total} kernels, {distinct} distinct")
    repeated = sorted(n for n, k in names.items() if k > 1)
    assert total == distinct, f"{len(repeated)} kernels in more than one code object, e.g. {repeated[:3]}"
