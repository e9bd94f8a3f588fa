"""Progressive JPEG (SOF2) on the device decoder, opt-in (`progressive=True`, reidmi_jpeg_plan_ex
with REIDMI_JPEG_PROGRESSIVE).  The oracle is the decoder the reference runs — Pillow 12.2 on
libjpeg-turbo, `Image.open(f).convert("RGB")` — which also writes the progressive files.  CPU
tests run the kernels' per-image code compiled for the host (tools/jpeg_host_check.hip: the same
lines of csrc/jpeg_core.h); GPU tests decode on the device."""
import ctypes
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image, ImageFile

from conftest import REPO
from multimodal_reid_amd import _lib, build_lib, data_prepare
from multimodal_reid_amd import synthetic as syn
from test_jpeg import _mutations, pil_rgb

VP = ctypes.c_void_p
KNOWN = {0, 1, 2, 3, 4, 5, 6}
SIZES = [(8, 8), (17, 9), (37, 23), (64, 32), (128, 64), (256, 128)]   # width x height
LAYOUTS = ["gray", 0, 1, 2]                                              # Pillow subsampling: 4:4:4, 4:2:2, 4:2:0


def prog_file(w, h, layout, seed=0, **kw):
    """One Pillow-written progressive file of a synthetic crop."""
    arr = syn.crop_rgb(h, w, seed, 1)
    b = io.BytesIO()
    # Pillow's progressive encoder needs an output buffer that holds the whole file (libjpeg
    # cannot suspend there); its default is too small for 256 x 128 at quality 100
    block, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, 1 << 22
    try:
        if layout == "gray":
            Image.fromarray(arr[:, :, 0]).save(b, "JPEG", progressive=True, **kw)
        else:
            Image.fromarray(arr).save(b, "JPEG", progressive=True, subsampling=layout, **kw)
    finally:
        ImageFile.MAXBLOCK = block
    return b.getvalue()


def matrix_cases():
    """The issue's matrix: sizes x {gray, 4:4:4, 4:2:2, 4:2:0} x quality x optimize x restart."""
    out = []
    for si, (w, h) in enumerate(SIZES):
        for layout in LAYOUTS:
            for q in (30, 75, 95, 100):
                for opt in (False, True):
                    for rst in (None, 1, 2):
                        kw = {"quality": q, "optimize": opt}
                        if rst:
                            kw["restart_marker_blocks"] = rst
                        out.append((f"{w}x{h}-{layout}-q{q}-opt{int(opt)}-rst{rst}",
                                    prog_file(w, h, layout, seed=si * 7 + q, **kw)))
    return out


def gpu_cases():
    """48 files of the matrix (every size, layout, quality, optimize and restart value
    occurs), for the device tests."""
    out = []
    k = 0
    for si, (w, h) in enumerate(SIZES):
        for layout in LAYOUTS:
            for j in range(2):
                q = (30, 75, 95, 100)[(k + j) % 4]
                rst = (None, 1, 2)[(k // 2 + j) % 3]
                kw = {"quality": q, "optimize": bool((k + j) % 2)}
                if rst:
                    kw["restart_marker_blocks"] = rst
                out.append((f"{w}x{h}-{layout}-q{q}-rst{rst}", prog_file(w, h, layout, seed=100 + k, **kw)))
            k += 1
    return out


def walk(b):
    """[(marker, start, end)] of a well-formed file: each segment with, for SOS, its entropy-coded
    data (to the next marker that is no RSTn and no stuffed 0xFF)."""
    out, p = [(0xD8, 0, 2)], 2
    while p < len(b):
        assert b[p] == 0xFF, p
        m = b[p + 1]
        if m == 0xD9:
            out.append((m, p, p + 2))
            break
        e = p + 2 + ((b[p + 2] << 8) | b[p + 3])
        if m == 0xDA:
            while not (b[e] == 0xFF and b[e + 1] != 0 and not 0xD0 <= b[e + 1] <= 0xD7):
                e += 1
        out.append((m, p, e))
        p = e
    return out


def _pil(b):
    """Pillow's image, or None where it raises."""
    try:
        return pil_rgb(b)
    except Exception:
        return None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tools/jpeg_host_check.hip built for the host, as test_jpeg.py builds it."""
    if not shutil.which(build_lib.HIPCC):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("jpeghost") / "libjpeghost.so")
    subprocess.run([build_lib.HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{build_lib.CSRC}",
                    f"-I{build_lib.INCLUDE}", os.path.join(REPO, "tools", "jpeg_host_check.hip"), "-o", so], check=True)
    return ctypes.CDLL(so)


def host_decode(host, files, progressive=True):
    """(JpegBatch, per-file status: the plan's, or the decode's where the plan took the file,
    pixels of the packed batch)."""
    jb = data_prepare.JpegBatch(files, progressive=progressive)
    out = np.zeros(max(jb.out_bytes, 1), np.uint8)
    err = np.zeros(max(jb.B, 1), np.int32)
    host.jpeg_host_decode(jb.buf.ctypes.data_as(VP), jb.plan.ctypes.data_as(VP), jb.info.ctypes.data_as(VP),
                          out.ctypes.data_as(VP), err.ctypes.data_as(VP))
    return jb, np.where(jb.status != 0, jb.status, err[:jb.B]), out


def image(jb, pix, k):
    off, h, w = jb.meta[k]
    return pix[off:off + h * w * 3].reshape(h, w, 3)


# ------------------------------------------------------------------ CPU: the host build of jpeg_core.h


def test_host_parity_with_pillow(host):
    cases = matrix_cases()
    assert len(cases) == 6 * 4 * 4 * 2 * 3
    jb, st, pix = host_decode(host, [b for _, b in cases])
    assert not st.any(), [(cases[k][0], int(st[k])) for k in np.nonzero(st)[0][:10]]
    assert int(jb.info[5]) >> 32 == len(cases)   # every one took the progressive path
    bad = [name for k, (name, b) in enumerate(cases) if not np.array_equal(image(jb, pix, k), pil_rgb(b))]
    assert not bad, (len(bad), bad[:10])


def plan_image(jb, k):
    """The int32 fields of image k's JpegImage in the plan blob (csrc/jpeg_core.h: 11 int64, then
    w, h, ncomp, cspace, mcux, mcuy, ri, status, hs[3], vs[3], bw[3], bh[3], dw[3], dh[3],
    quant[3], dc[3], ac[3], cid[3], scan0, nscan)."""
    img_off = int(jb.plan[:32].view(np.int64)[3])
    return jb.plan[img_off + 248 * k + 88:img_off + 248 * (k + 1)].view(np.int32)


def test_block_geometry_of_noninterleaved_scans(host):
    """37 x 23 at 4:2:0: the interleaved DC scan walks the 3 x 2 MCU grid (6 x 4 luma blocks),
    the luma AC scans the 5 x 3 blocks of the 37 x 23 component.  The plan holds those numbers,
    the file has one three-component scan and single-component ones, and the pixels are Pillow's."""
    b = prog_file(37, 23, 2, seed=3, quality=90)
    jb, st, pix = host_decode(host, [b])
    assert st.tolist() == [0] and np.array_equal(image(jb, pix, 0), pil_rgb(b))
    f = plan_image(jb, 0).tolist()
    assert f[4:6] == [3, 2] and f[14:20] == [6, 3, 3, 4, 2, 2]          # mcux, mcuy; bw[], bh[]
    assert f[20:26] == [37, 19, 19, 23, 12, 12] and f[39] == 10         # dw[], dh[]; nscan
    assert ((f[20] + 7) // 8, (f[23] + 7) // 8) == (5, 3)
    scans = [s for s in walk(b) if s[0] == 0xDA]
    assert len(scans) == 10 and b[scans[0][1] + 4] == 3 and b[scans[1][1] + 4] == 1


def test_quantiser_redefined_between_scans_is_latched_at_first_use(host):
    """A DQT between two scans that redefines the tables of components already seen: libjpeg keeps
    the table that was current at a component's first scan (latch_quant_tables), so Pillow returns
    the image of the unchanged file — and so must the decode."""
    for layout in (2, "gray"):
        b = prog_file(64, 32, layout, seed=9, quality=75)
        end1 = [e for m, _, e in walk(b) if m == 0xDA][0]
        dqt = b"".join(b"\xff\xdb\x00\x43" + bytes([t]) + bytes([99] * 64) for t in (0, 1))
        mod = b[:end1] + dqt + b[end1:]
        ref = pil_rgb(mod)
        assert np.array_equal(ref, pil_rgb(b))   # (Pillow latches)
        jb, st, pix = host_decode(host, [mod])
        assert st.tolist() == [0] and np.array_equal(image(jb, pix, 0), ref)


def refused_sof2():
    """A progressive file the planner refuses only after its marker walk: the SOF2 luma sampling
    set to 1 x 2 (4:4:0, status 3: a layout the device does not decode)."""
    b = bytearray(prog_file(64, 32, 2, seed=62, quality=75))
    p = next(s for m, s, _ in walk(bytes(b)) if m == 0xC2)
    assert b[p + 11] == 0x22
    b[p + 11] = 0x12
    return bytes(b)


def test_refused_progressive_file_is_no_progressive_image_in_the_plan():
    good = prog_file(64, 32, 2, seed=60, quality=75)
    jb = data_prepare.JpegBatch([refused_sof2(), good], progressive=True)
    assert jb.status.tolist() == [3, 0] and int(jb.info[5]) >> 32 == 1
    assert plan_image(jb, 0)[38:40].tolist() == [0, 0] and plan_image(jb, 1)[39] == 10


@pytest.mark.parametrize("layout", ["gray", 2])
def test_every_prefix_cut_fails_exactly_where_pillow_raises(host, layout):
    b = prog_file(64, 48, "gray", seed=5, quality=75) if layout == "gray" else prog_file(40, 24, 2, seed=5, quality=75)
    assert 700 < len(b) < 1300, len(b)   # about 1 KB: one file per prefix
    cuts = [b[:n] for n in range(len(b) + 1)]
    _, st, _ = host_decode(host, cuts)
    assert set(st.tolist()) <= KNOWN
    ref = [_pil(c) is None for c in cuts]
    mism = [(n, int(st[n]), ref[n]) for n in range(len(cuts)) if (st[n] != 0) != ref[n]]
    assert not mism, mism[:10]
    assert st[-1] == 0 and st[:-1].all()   # (and Pillow agrees: only the whole file loads)
    assert (st == 6).any() and (st == 1).any()


@pytest.mark.parametrize("layout", ["gray", 2])
def test_incomplete_scan_scripts_are_unsupported(host, layout):
    """The file cut after its k-th scan with EOI appended is a legal file whose scan script stops
    short of full precision: status 2 for every k below the full count, 0 for the whole file."""
    b = prog_file(40, 24, layout, seed=6, quality=75)
    segs = walk(b)
    ends = [e for m, _, e in segs if m == 0xDA]
    assert len(ends) == (6 if layout == "gray" else 10)
    files = [b[:e] + b"\xff\xd9" for e in ends[:-1]] + [b]
    _, st, _ = host_decode(host, files)
    assert st.tolist() == [2] * (len(ends) - 1) + [0]
    assert all(_pil(f) is not None for f in files)   # (Pillow returns an approximation of these)


def _plan(name, files, *flags):
    buf, off = data_prepare.read_files(files)
    B = len(files)
    meta, status, info = np.zeros((B, 3), np.int64), np.zeros(B, np.int32), np.zeros(10, np.int64)
    args = (buf.ctypes.data_as(VP), off.ctypes.data_as(VP), B) + flags
    _lib.call(name, *args, None, 0, meta.ctypes.data_as(VP), status.ctypes.data_as(VP), info.ctypes.data_as(VP))
    plan = np.zeros(int(info[0]), np.uint8)
    _lib.call(name, *args, plan.ctypes.data_as(VP), plan.size, meta.ctypes.data_as(VP), status.ctypes.data_as(VP),
              info.ctypes.data_as(VP))
    return status, meta, info, plan


def test_default_path_is_unchanged(host):
    base = syn.jpeg_files(3, 128, 64, seed=1) + syn.jpeg_files(1, 37, 29, seed=2, subsampling=1, restart_marker_blocks=2)
    prog = [prog_file(64, 32, 2, seed=7), prog_file(17, 9, "gray", seed=8)]
    cmyk = io.BytesIO()
    Image.fromarray(syn.crop_rgb(16, 16, 3)).convert("CMYK").save(cmyk, "JPEG")
    files = [base[0], prog[0], b"not a jpeg", base[1], cmyk.getvalue(), base[2][:40], prog[1], base[3], base[2][:-300]]
    old = _plan("reidmi_jpeg_plan", files)
    new = _plan("reidmi_jpeg_plan_ex", files, 0)
    for a, b in zip(old, new):
        assert np.array_equal(a, b)
    assert old[0].tolist() == [0, 2, 1, 0, 3, 1, 2, 0, 0]
    # with the flag: the progressive files are planned, the baseline ones are as they were
    jb0, st0, pix0 = host_decode(host, files, progressive=False)
    jb1, st1, pix1 = host_decode(host, files, progressive=True)
    assert jb1.status.tolist() == [0, 0, 1, 0, 3, 1, 0, 0, 0] and int(jb1.info[5]) >> 32 == 2
    assert st1.tolist() == [0, 0, 1, 0, 3, 1, 0, 0, 6]
    for k in (0, 3, 7, 8):
        assert st0[k] == st1[k] and jb0.meta[k, 1:].tolist() == jb1.meta[k, 1:].tolist()
        assert np.array_equal(image(jb0, pix0, k), image(jb1, pix1, k))
    for k in (1, 6):
        assert np.array_equal(image(jb1, pix1, k), pil_rgb(files[k]))
    with pytest.raises(_lib.ReidmiError, match="unknown flags"):
        _plan("reidmi_jpeg_plan_ex", files, 2)


def damaged_progressive(n=320, seed=9):
    """Random cuts, bit flips, overwritten runs and inserted 0xFF / marker bytes (test_jpeg.py's
    kinds of damage) of progressive files of every layout, with and without restart intervals."""
    seeds = [prog_file(64, 32, 2, seed=20, quality=75), prog_file(37, 23, 2, seed=21, quality=95, optimize=True),
             prog_file(64, 32, 1, seed=22, quality=75, restart_marker_blocks=2), prog_file(17, 9, 0, seed=23, quality=100),
             prog_file(37, 23, "gray", seed=24, quality=75, restart_marker_blocks=1),
             prog_file(128, 64, 2, seed=25, quality=30), prog_file(64, 32, 0, seed=26, quality=75, optimize=True),
             prog_file(8, 8, 1, seed=27, quality=75)]
    return _mutations(seeds, n, seed)


def test_damaged_files_terminate_with_a_known_status(host):
    """Termination and a status of the known set are asserted; parity with Pillow on damaged
    progressive data is not claimed — the count of disagreements is printed (recorded in DESIGN.md §5)."""
    dm = damaged_progressive()
    jb, st, pix = host_decode(host, dm)
    assert set(st.tolist()) <= KNOWN
    ref = [_pil(b) for b in dm]
    differ = sum(1 for k in range(len(dm)) if st[k] == 0 and ref[k] is not None
                 and not np.array_equal(image(jb, pix, k), ref[k]))
    raises = sum(1 for k in range(len(dm)) if st[k] == 0 and ref[k] is None)
    print(f"damaged progressive files: {len(dm)}, statuses {np.bincount(st, minlength=7).tolist()}, "
          f"status 0 with pixels other than Pillow's: {differ}, status 0 where Pillow raises: {raises}")
    assert (st == 0).any() and (st != 0).any()


def test_progressive_host_code_under_asan_ubsan(host, tmp_path):
    """The planner with the progressive flag and the progressive decode as a stand-alone
    executable (tools/jpeg_prog_asan_main.hip) under AddressSanitizer + UBSan, every report fatal,
    over the damaged files and a slice of the parity matrix: a clean exit, and the answers of
    the unsanitised build."""
    exe = str(tmp_path / "jpeg_prog_asan")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g"]
    subprocess.run([build_lib.HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", *san, f"-I{build_lib.CSRC}",
                    f"-I{build_lib.INCLUDE}", os.path.join(REPO, "tools", "jpeg_prog_asan_main.hip"), "-o", exe],
                   check=True)
    files = damaged_progressive() + [b for _, b in matrix_cases()[::7]] + [b"", b"\xff", b"\xff\xd8\xff"]
    jb, st, pix = host_decode(host, files)
    blob = struct.pack("<q", len(files)) + np.asarray(jb.offsets, np.int64).tobytes() + jb.buf.tobytes()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], input=blob, capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-4000:]
    B, out = len(files), r.stdout
    status = np.frombuffer(out, np.int32, B, 0)
    meta = np.frombuffer(out, np.int64, 3 * B, 4 * B).reshape(B, 3)
    info = np.frombuffer(out, np.int64, 10, 28 * B)
    err = np.frombuffer(out, np.int32, B, 28 * B + 80)
    got = np.frombuffer(out, np.uint8, int(info[2]), 32 * B + 80)
    assert np.array_equal(status, jb.status) and np.array_equal(meta, jb.meta) and np.array_equal(info, jb.info)
    assert np.array_equal(np.where(status != 0, status, err), st)
    assert np.array_equal(got, pix[:jb.out_bytes])
    print(f"progressive jpeg under ASan/UBSan: {B} files, statuses {np.bincount(st, minlength=7).tolist()}")


def test_keyword_defaults_refuse_progressive():
    """Opt-in: without the keyword a progressive file keeps status 2 and its text."""
    b = prog_file(64, 32, 2, seed=30)
    assert data_prepare.JpegBatch([b]).status.tolist() == [2]
    assert data_prepare.JpegBatch([b], progressive=True).status.tolist() == [0]
    assert data_prepare.JPEG_STATUS[2].startswith("progressive")


# ------------------------------------------------------------------ GPU: device decode vs Pillow


@pytest.fixture(scope="module")
def mixed():
    """~40 progressive files of the matrix shuffled with baseline files: (names, files,
    indices of the baseline ones, Pillow's images) — computed once, left unchanged."""
    cases = gpu_cases() + [(f"base{k}", b) for k, b in enumerate(
        syn.jpeg_files(6, 128, 64, seed=31) + syn.jpeg_files(2, 37, 29, seed=32, subsampling=1)
        + syn.jpeg_files(2, 77, 45, seed=33, restart_marker_rows=1))]
    order = np.random.default_rng(5).permutation(len(cases))
    cases = [cases[k] for k in order]
    files = [b for _, b in cases]
    base = [k for k, (name, _) in enumerate(cases) if name.startswith("base")]
    return [n for n, _ in cases], files, base, [pil_rgb(b) for b in files]


@pytest.mark.gpu
def test_gpu_mixed_batch_bitexact_vs_pillow(gpu, mixed):
    names, files, base, ref = mixed
    pix, meta, jb = data_prepare.decode_jpeg(files, progressive=True)
    torch.cuda.synchronize()
    pix = pix.cpu().numpy()
    assert int(jb.info[5]) >> 32 == len(files) - len(base)
    bad = [names[k] for k in range(len(files)) if not np.array_equal(image(jb, pix, k), ref[k])]
    assert not bad, bad
    assert np.array_equal(meta.cpu().numpy(), jb.meta)


@pytest.mark.gpu
def test_gpu_sequential_path_not_perturbed(gpu, mixed):
    """The baseline images of the mixed batch are what decode_jpeg of the baseline files alone
    returns (the default path, which launches nothing new)."""
    _, files, base, _ = mixed
    pix, _, jb = data_prepare.decode_jpeg(files, progressive=True)
    alone, _, ja = data_prepare.decode_jpeg([files[k] for k in base])
    torch.cuda.synchronize()
    pix, alone = pix.cpu().numpy(), alone.cpu().numpy()
    assert int(ja.info[5]) >> 32 == 0
    for j, k in enumerate(base):
        assert np.array_equal(image(jb, pix, k), image(ja, alone, j)), k


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_gpu_preprocess_jpeg_progressive_equals_pil_pipeline(gpu, dtype):
    files = [prog_file(64, 128, 2, seed=40 + k, quality=75) for k in range(24)]   # Market-size crops: 128 high, 64 wide
    a = data_prepare.preprocess_jpeg(files, dtype=dtype, progressive=True)
    b = data_prepare.preprocess([Image.open(io.BytesIO(f)) for f in files], dtype=dtype)
    assert torch.equal(a.view(torch.int16 if dtype == torch.float16 else torch.int32),
                       b.view(torch.int16 if dtype == torch.float16 else torch.int32))


@pytest.mark.gpu
def test_gpu_loader_progressive_equals_per_call_path(gpu):
    class _DS:
        pass
    prog = [prog_file(64, 128, (2, 1, 0, "gray")[k % 4], seed=50 + k, quality=80, optimize=bool(k % 2)) for k in range(9)]
    base = syn.jpeg_files(8, 128, 64, seed=51)
    files = [f for pair in zip(prog, base) for f in pair] + prog[8:]
    ds = _DS()
    ds.gallery = [(f, k, k % 3, 0, k) for k, f in enumerate(files)]
    ds.query = [(f, k, k % 2, 0, k) for k, f in enumerate(files[:5])]
    g, q, _, _ = data_prepare.get_loader(ds, 7, 256, 128, "vit", progressive=True)
    for loader, items in ((g, ds.gallery), (q, ds.query)):
        got = torch.cat([batch[0] for batch in loader])
        want = data_prepare.preprocess_jpeg([it[0] for it in items], progressive=True)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # and without the keyword the same list raises at its first batch
    g0 = data_prepare.get_loader(ds, 7, 256, 128, "vit")[0]
    with pytest.raises(ValueError, match="progressive"):
        next(iter(g0))


def corrupt_entropy(b):
    """One fixed corruption of a progressive file: every 7th byte of its third scan's
    entropy-coded data flipped or made 0xFF (the damage of test_jpeg.py's bad-data test)."""
    scans = [(s, e) for m, s, e in walk(b) if m == 0xDA]
    s, e = scans[2]
    s += 2 + ((b[s + 2] << 8) | b[s + 3])
    bad = bytearray(b)
    for k in range(s + 3, e - 1, 7):
        bad[k] = 0xFF if bad[k + 1] == 0 else bad[k] ^ 0x5A
    return bytes(bad)


def test_corrupt_entropy_survives_on_the_host(host):
    """The corruption the GPU test uses, through the host build of the same code first."""
    good = prog_file(64, 32, 2, seed=60, quality=75)
    jb, st, pix = host_decode(host, [good, corrupt_entropy(good)])
    assert st[0] == 0 and int(st[1]) in KNOWN and jb.status.tolist() == [0, 0]
    assert np.array_equal(image(jb, pix, 0), pil_rgb(good))


@pytest.mark.gpu
def test_gpu_damaged_file_beside_a_good_one(gpu):
    good = prog_file(64, 32, 2, seed=60, quality=75)
    pix, _, jb, err = data_prepare.decode_jpeg([good, corrupt_entropy(good)], check=False, return_status=True,
                                               progressive=True)
    torch.cuda.synchronize()
    err = err.cpu().numpy()
    assert err[0] == 0 and int(err[1]) in KNOWN
    assert np.array_equal(image(jb, pix.cpu().numpy(), 0), pil_rgb(good))


@pytest.mark.gpu
def test_gpu_planner_refused_progressive_file_reports_its_plan_status(gpu):
    """A SOF2 file refused after the marker walk, beside a good one, unchecked: the device status
    of every file is written and equals the plan status."""
    good = prog_file(64, 32, 2, seed=60, quality=75)
    files = [good, refused_sof2(), syn.jpeg_files(1, 40, 24, seed=63)[0], refused_sof2()]
    pix, _, jb, err = data_prepare.decode_jpeg(files, check=False, return_status=True, progressive=True)
    torch.cuda.synchronize()
    assert jb.status.tolist() == [0, 3, 0, 3] and err.cpu().numpy().tolist() == [0, 3, 0, 3]
    pix = pix.cpu().numpy()
    for k in (0, 2):
        assert np.array_equal(image(jb, pix, k), pil_rgb(files[k]))
    only = data_prepare.decode_jpeg([refused_sof2()], check=False, return_status=True, progressive=True)[3]
    assert only.cpu().numpy().tolist() == [3]


@pytest.mark.gpu
def test_gpu_incomplete_scan_script_raises_unsupported(gpu):
    b = prog_file(64, 32, 2, seed=61, quality=75)
    ends = [e for m, _, e in walk(b) if m == 0xDA]
    cut = b[:ends[2]] + b"\xff\xd9"
    with pytest.raises(ValueError, match="progressive / lossless"):
        data_prepare.decode_jpeg([syn.jpeg_files(1, 8, 8)[0], cut], progressive=True)
