"""Build libofx.so (the C-ABI HIP library) for gfx950 with hipcc, in-tree.

    python -m octfusion_amd.build [--force]

hipcc cross-compiles without a GPU.  Every translation unit is compiled to its own object (in parallel) and the
objects are linked into the shared library.  Rebuilds are decided by CONTENT, not by mtime: an object carries the
sha256 of its source, every header and the flags it was built from (``<obj>.sha``), and the library embeds the hash
of the whole source set (``ofx_build_hash()``), which ``octfusion_amd._lib`` compares with the tree before the
first call -- a stale ``libofx.so`` (the file is git-ignored and travels with the gpurun snapshot) is refused
instead of silently run.
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(CSRC, '_obj')
LIB = os.path.join(HERE, 'libofx.so')
SOURCES = ['ofx_octree.hip', 'ofx_graph.hip', 'ofx_gemm.hip', 'ofx_gemm2.hip', 'ofx_gemm3.hip', 'ofx_norm.hip',
           'ofx_dense.hip', 'ofx_misc.hip', 'ofx_loss.hip', 'ofx_points.hip', 'ofx_probe.hip', 'ofx_narrow.hip',
           'ofx_mesh.hip', 'ofx_mesh_cc.hip', 'ofx_metrics.hip', 'ofx_voxmesh.hip', 'ofx_sdfdata.hip',
           'ofx_mesh2sdf.hip', 'ofx_train.hip', 'ofx_render.hip', 'ofx_nnsearch.hip',
           'ofx_simplify.hip', 'ofx_fieldmesh.hip', 'ofx_normals.hip', 'ofx_tribins.hip', 'ofx_meshquery.hip',
           'ofx_raycast.hip', 'ofx_winding.hip', 'ofx_meshcheck.hip', 'ofx_meshsmooth.hip']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC']


def _headers():
    hs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h'))
    hs.append(os.path.join(os.path.dirname(HERE), 'include', 'ofx.h'))
    return hs


def _sha(paths, extra=()):
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode() + b'\0')
        with open(p, 'rb') as f:
            h.update(f.read())
        h.update(b'\0')
    for e in extra:
        h.update(e.encode() + b'\0')
    return h.hexdigest()


def source_hash():
    """sha256 (first 16 hex digits) of every source, header and compile flag of the library."""
    return _sha([os.path.join(CSRC, s) for s in SOURCES] + _headers(), FLAGS)[:16]


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return None


def build(force=False, verbose=False):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    os.makedirs(OBJ, exist_ok=True)
    hdrs = _headers()
    jobs, objs, stamps = [], [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s.replace('.hip', '.o'))
        want = _sha([src] + hdrs, FLAGS)
        objs.append(obj)
        if force or not os.path.exists(obj) or _read(obj + '.sha') != want:
            jobs.append([hipcc] + FLAGS + ['-c', src, '-o', obj])
            stamps.append((obj + '.sha', want))

    def run(cmd):
        if verbose:
            print(' '.join(cmd))
        subprocess.run(cmd, check=True)
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(run, jobs))
        for path, want in stamps:
            with open(path, 'w') as f:
                f.write(want)
    # the hash of the whole source set, compiled into the library
    tree = source_hash()
    info_c = os.path.join(OBJ, 'ofx_buildinfo.cpp')
    info_o = os.path.join(OBJ, 'ofx_buildinfo.o')
    text = 'extern "C" const char* ofx_build_hash() { return "%s"; }\n' % tree
    relink = bool(jobs) or force or not os.path.exists(LIB)
    if _read(info_c) != text.strip() or not os.path.exists(info_o):
        with open(info_c, 'w') as f:
            f.write(text)
        run([hipcc, '-O2', '-fPIC', '-c', info_c, '-o', info_o])
        relink = True
    if relink:
        run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs + [info_o])
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
