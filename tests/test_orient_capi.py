"""CPU: the EXIF orientation's C interface -- the tag readers over well-formed, odd and damaged files (in process, and as a stand-alone
program under the address and undefined-behaviour sanitizers), the size / rectangle / inverse helpers against the table in numpy, the
stage's per-lane bodies on the CPU under the sanitizers, every refusal of ffhip_bgra_orient_items and the oriented file calls before the
device is asked for, and the tag and the upright size against PIL."""
import ctypes as C
import io
import itertools
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import exif_cases as X
from ffpic_amd import capi, ops, tensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL, ENODEV = capi.FFHIP_EINVAL, capi.FFHIP_ENODEV
AA = capi.FFHIP_RESIZE_ANTIALIAS


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


@pytest.fixture(scope="module")
def jpeg():
    return X.writer_jpeg(np.random.default_rng(3), 37, 23, "420")


@pytest.fixture(scope="module")
def webp():
    return open(os.path.join(GOLDEN, "pil_50x48_q30.webp"), "rb").read()


def read(L, data, webp=False):
    """(return code, orientation) of the bytes, from a buffer of exactly their length"""
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\x00")
    o = C.c_int(-1)
    rc = (L.ffhip_webp_exif_orientation if webp else L.ffhip_jpeg_exif_orientation)(buf, len(data), C.byref(o))
    return rc, o.value


# ---------------------------------------------------------------------------------------------------- the tag
def test_struct_layout_and_declarations_match_the_header():
    text = open(os.path.join(ROOT, "include", "ffpic_hip.h")).read()
    I = capi.OrientItem
    assert C.sizeof(I) == 56
    assert (I.d_src.offset, I.src_pitch.offset, I.x0.offset, I.y0.offset, I.width.offset, I.height.offset) == (0, 8, 16, 20, 24, 28)
    assert (I.d_dst.offset, I.dst_pitch.offset, I.orientation.offset) == (32, 40, 48)
    body = re.search(r"typedef struct ffhip_orient_item \{(.*?)\} ffhip_orient_item;", text, flags=re.S).group(1)
    at = [body.index(f) for f in ("d_src", "src_pitch", "x0", "height", "d_dst", "dst_pitch", "orientation")]
    assert at == sorted(at)
    for entry in ("ffhip_jpeg_exif_orientation", "ffhip_webp_exif_orientation", "ffhip_orient_size", "ffhip_orient_rect", "ffhip_orient_inverse",
                  "ffhip_bgra_orient_items", "ffhip_jpeg_decode_files_tensor_oriented", "ffhip_webp_decode_files_tensor_oriented",
                  "ffhip_debug_orient_last_items"):
        assert entry in capi.EXPORTS and re.search(r"\b" + entry + r"\(", text), entry


@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("kind", [X.SHORT, X.LONG])
def test_every_value_in_both_byte_orders_types_and_containers(L, jpeg, webp, big_endian, kind):
    for o in range(1, 9):
        assert read(L, X.tagged_jpeg(jpeg, o, big_endian=big_endian, kind=kind)) == (0, o)
        assert ops.jpeg_exif_orientation(X.tagged_jpeg(jpeg, o, big_endian=big_endian, kind=kind, before=0, after=0)) == o
        for prefix in (False, True):
            assert read(L, X.tagged_webp(webp, o, exif_prefix=prefix, big_endian=big_endian, kind=kind), webp=True) == (0, o)
        assert ops.webp_exif_orientation(X.tagged_webp(webp, o, big_endian=big_endian, kind=kind, before=3, after=0)) == o
    # an IFD that does not follow the header directly
    assert read(L, X.tagged_jpeg(jpeg, 6, big_endian=big_endian, kind=kind, ifd_offset=26)) == (0, 6)


def test_the_tagged_files_still_decode_to_the_same_size(L, jpeg, webp):
    g, w, h = ops.jpeg_probe(jpeg)
    g2, w2, h2 = ops.jpeg_probe(X.tagged_jpeg(jpeg, 6))
    assert (w, h, g.mcu_cols, g.mcu_rows) == (w2, h2, g2.mcu_cols, g2.mcu_rows) == (37, 23, 3, 2)
    for name in ("pil_50x48_q30", "syn_vp8x", "pil_17x16_q50"):
        data = open(os.path.join(GOLDEN, name + ".webp"), "rb").read()
        assert ops.webp_probe(X.tagged_webp(data, 8)) == ops.webp_probe(data), name


def test_files_without_a_usable_tag_give_1(L, jpeg, webp):
    def ifd_at(offset):
        """a good structure whose header points somewhere else"""
        return X.splice(jpeg, X.app1(b"Exif\x00\x00" + X.tiff(6)[:4] + struct.pack("<I", offset) + X.tiff(6)[8:]))
    assert read(L, ifd_at(8)) == (0, 6)
    cases = {
        "no APP1": jpeg,
        "an APP1 that is XMP": X.splice(jpeg, X.XMP_APP1),
        "value 0": X.tagged_jpeg(jpeg, 0),
        "value 9": X.tagged_jpeg(jpeg, 9),
        "value 65542 as LONG": X.tagged_jpeg(jpeg, 65536 + 6, kind=X.LONG),
        "count 2": X.tagged_jpeg(jpeg, 6, count=2),
        "count 0": X.tagged_jpeg(jpeg, 6, count=0),
        "type BYTE": X.tagged_jpeg(jpeg, 6, kind=1),
        "another tag only": X.tagged_jpeg(jpeg, 6, tag=0x0113),
        "IFD offset outside the segment": ifd_at(4000),
        "IFD offset far outside the segment": ifd_at(0xFFFFFFF0),
        "IFD offset at the segment's last byte": ifd_at(len(X.tiff(6)) - 1),
        "IFD offset at the segment's end": ifd_at(len(X.tiff(6))),
        "more entries than the segment holds": X.tagged_jpeg(jpeg, 6, before=0, after=0, n_entries=200),
        "an unknown byte order": X.splice(jpeg, X.app1(b"Exif\x00\x00" + b"IM\x2a\x00" + X.tiff(6)[4:])),
        "an Exif header and nothing else": X.splice(jpeg, X.app1(b"Exif\x00\x00")),
        "not a JPEG": b"\x00\x01\x02\x03" + X.exif_app1(6),
        "empty": b"",
        "SOI only": b"\xff\xd8",
        "a tag behind SOS": jpeg[:-2] + X.exif_app1(6) + jpeg[-2:],
    }
    tagged = X.tagged_jpeg(jpeg, 6)
    seg_len = struct.unpack(">H", tagged[4:6])[0]
    cases["a segment length running past the file"] = tagged[:2 + 2 + seg_len - 3]
    cases["a segment length running far past the file"] = tagged[:4] + b"\xff\xff" + tagged[6:40]
    for name, data in cases.items():
        assert read(L, data) == (0, 1), name
    # two of them only mean something if the tag WOULD be found otherwise
    assert read(L, X.tagged_jpeg(jpeg, 6, before=0, after=0)) == (0, 6)
    wcases = {
        "no EXIF chunk": webp,
        "value 9": X.tagged_webp(webp, 9),
        "count 2": X.tagged_webp(webp, 6, count=2),
        "more entries than the chunk holds": X.tagged_webp(webp, 6, n_entries=99),
        "a chunk size running past the file": X.tagged_webp(webp, 6)[:-3],
        "not a RIFF file": b"RIFX" + X.tagged_webp(webp, 6)[4:],
        "a JPEG": tagged,
        "empty": b"",
    }
    for name, data in wcases.items():
        assert read(L, data, webp=True) == (0, 1), name


def test_a_tag_behind_another_app1_and_the_first_exif_decides(L, jpeg):
    assert read(L, X.splice(jpeg, X.XMP_APP1, X.exif_app1(7))) == (0, 7)
    assert read(L, X.splice(jpeg, X.app1(b"Exi"), X.XMP_APP1, b"\xff\xe0" + struct.pack(">H", 16) + b"JFIF\x00" + bytes(9), X.exif_app1(5, big_endian=True))) == (0, 5)
    assert read(L, X.splice(jpeg, X.exif_app1(3), X.exif_app1(6))) == (0, 3)
    assert read(L, X.splice(jpeg, X.exif_app1(9), X.exif_app1(6))) == (0, 1)          # the first one decides, usable or not
    assert read(L, X.splice(jpeg, b"\xff\xff\xff" + X.exif_app1(4)[1:])) == (0, 4)    # fill bytes in front of a marker


def test_null_arguments_are_the_only_refusal(L, jpeg):
    buf = (C.c_uint8 * len(jpeg)).from_buffer_copy(jpeg)
    o = C.c_int(5)
    for f in (L.ffhip_jpeg_exif_orientation, L.ffhip_webp_exif_orientation):
        assert f(None, len(jpeg), C.byref(o)) == EINVAL and f(buf, len(jpeg), None) == EINVAL
        assert f(buf, 0, C.byref(o)) == 0 and o.value == 1


@pytest.mark.parametrize("container", ["jpeg", "webp"])
def test_every_truncation_and_every_mutation_of_the_exif_block(L, jpeg, webp, container):
    """FFHIP_OK and a value in 1..8, whatever is done to the file"""
    is_webp = container == "webp"
    for big_endian, kind in itertools.product((False, True), (X.SHORT, X.LONG)):
        data = X.tagged_webp(webp, 6, big_endian=big_endian, kind=kind) if is_webp else X.tagged_jpeg(jpeg, 6, big_endian=big_endian, kind=kind)
        assert read(L, data, is_webp) == (0, 6)
        for cut in range(len(data) + 1):
            rc, o = read(L, data[:cut], is_webp)
            assert rc == 0 and 1 <= o <= 8, cut
        if is_webp:
            first = data.index(b"EXIF")
            end = len(data)
        else:
            first, end = 2, 4 + struct.unpack(">H", data[4:6])[0]
        f = L.ffhip_webp_exif_orientation if is_webp else L.ffhip_jpeg_exif_orientation
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        o, seen = C.c_int(), set()
        for at in range(first, end):
            keep = buf[at]
            for v in range(256):
                if v == keep:
                    continue
                buf[at] = v
                assert f(buf, len(data), C.byref(o)) == 0 and 1 <= o.value <= 8, (at, v)
                seen.add(o.value)
            buf[at] = keep
        assert seen == set(range(1, 9))                                        # the mutations reach the value itself


def _sanitizer_build(tmp_path, sources, out, compiler, flags=()):
    cc = shutil.which(compiler)
    if not cc:
        pytest.skip(f"no {compiler}")
    probe = tmp_path / ("probe" + (".cc" if compiler == "c++" else ".c"))
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run([cc, "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    exe = tmp_path / out
    subprocess.run([cc, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *flags, "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "ffpic_amd", "csrc"), *sources, "-o", str(exe)], check=True)
    return str(exe)


def test_sanitizer_program_over_truncated_and_mutated_files(tmp_path, jpeg, webp):
    """ffhip_exif.c and tests/tools/exif_fuzz_main.c as a program of their own under ASan + UBSan: exit 0, nothing on stderr"""
    csrc = os.path.join(ROOT, "ffpic_amd", "csrc")
    exe = _sanitizer_build(tmp_path, [os.path.join(csrc, "ffhip_exif.c"), os.path.join(csrc, "ffhip_jpeg_front.c"), os.path.join(ROOT, "tests", "tools", "exif_fuzz_main.c")],
                           "exif_fuzz", "cc", ["-std=c11"])
    files = {"le_short.jpg": X.tagged_jpeg(jpeg, 6), "be_long.jpg": X.tagged_jpeg(jpeg, 8, big_endian=True, kind=X.LONG),
             "behind_xmp.jpg": X.splice(jpeg, X.XMP_APP1, X.exif_app1(3)), "plain.jpg": jpeg,
             "le_short.webp": X.tagged_webp(webp, 6), "be_long_prefixed.webp": X.tagged_webp(webp, 5, exif_prefix=True, big_endian=True, kind=X.LONG),
             "plain.webp": webp}
    paths = []
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
        paths.append(str(tmp_path / name))
    run = subprocess.run([exe, *paths], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stderr == b"" and run.stdout == b"", run.stderr.decode(errors="replace")[-2000:]


def test_stage_bodies_on_the_cpu_under_sanitizers(tmp_path):
    """the kernel's per-lane bodies (ffhip_orient_body.h), lane by lane in the kernel's order over exact-size allocations, every size of
    the GPU test and all eight orientations: no read outside the stored picture, no write outside the upright one, the table's pixels"""
    exe = _sanitizer_build(tmp_path, [os.path.join(ROOT, "tests", "tools", "orient_body_main.cc")], "orient_body", "c++", ["-std=c++17"])
    run = subprocess.run([exe], capture_output=True, timeout=600)
    assert run.returncode == 0 and run.stderr == b"" and run.stdout == b"", run.stderr.decode(errors="replace")[-2000:]


# ---------------------------------------------------------------------------------------------------- sizes, rectangles, inverses
def lib_rect(L, ws, hs, o, rect):
    out = capi.Rect(-1, -1, -1, -1)
    rc = L.ffhip_orient_rect(ws, hs, o, C.byref(capi.Rect(*rect)), C.byref(out))
    return rc, (out.x0, out.y0, out.width, out.height)


def test_the_numpy_table_is_the_header_s_table():
    """U[y][x] as the header writes it, pixel by pixel, on a picture of distinct values"""
    ws, hs = 5, 3
    S = np.arange(ws * hs).reshape(hs, ws, 1)
    rule = {1: lambda x, y: (y, x), 2: lambda x, y: (y, ws - 1 - x), 3: lambda x, y: (hs - 1 - y, ws - 1 - x), 4: lambda x, y: (hs - 1 - y, x),
            5: lambda x, y: (x, y), 6: lambda x, y: (hs - 1 - x, y), 7: lambda x, y: (hs - 1 - x, ws - 1 - y), 8: lambda x, y: (x, ws - 1 - y)}
    for o in range(1, 9):
        U = X.orient(S, o)
        uw, uh = X.upright_size(ws, hs, o)
        assert U.shape[:2] == (uh, uw)
        for y, x in itertools.product(range(uh), range(uw)):
            assert U[y, x, 0] == S[rule[o](x, y) + (0,)], (o, x, y)


def test_size_rect_and_inverse_against_the_table(L):
    rng = np.random.default_rng(5)
    shapes = [(1, 1), (1, 9), (9, 1), (7, 5), (64, 65), (130, 67)]
    for (ws, hs), o in itertools.product(shapes, range(1, 9)):
        S = rng.integers(0, 256, (hs, ws, 4), dtype=np.uint8)
        U = X.orient(S, o)
        assert ops.orient_size(ws, hs, o) == (U.shape[1], U.shape[0]) == X.upright_size(ws, hs, o)
        uw, uh = U.shape[1], U.shape[0]
        rects = [(0, 0, uw, uh), (0, 0, 1, 1), (uw - 1, uh - 1, 1, 1)]
        for _ in range(12):
            w, h = int(rng.integers(1, uw + 1)), int(rng.integers(1, uh + 1))
            rects.append((int(rng.integers(0, uw - w + 1)), int(rng.integers(0, uh - h + 1)), w, h))
        for r in rects:
            rc, (sx, sy, sw, sh) = lib_rect(L, ws, hs, o, r)
            assert rc == 0 and (sx, sy, sw, sh) == X.stored_rect(ws, hs, o, r) == ops.orient_rect(ws, hs, o, r), (ws, hs, o, r)
            x0, y0, w, h = r
            assert np.array_equal(U[y0:y0 + h, x0:x0 + w], X.orient(S[sy:sy + sh, sx:sx + sw], o)), (ws, hs, o, r)
        # the inverse brings the picture back
        inv = ops.orient_inverse(o)
        assert inv == X.INVERSE[o] and np.array_equal(X.orient(U, inv), S)
    assert lib_rect(L, 40, 30, 6, (1, 2, 5, 7)) == (0, (2, 30 - 1 - 5, 7, 5))                     # the header's example


def test_helper_refusals(L):
    w, h, r = C.c_int(), C.c_int(), capi.Rect()
    for o in (0, 9, -1):
        assert L.ffhip_orient_size(4, 3, o, C.byref(w), C.byref(h)) == EINVAL
        assert L.ffhip_orient_rect(4, 3, o, C.byref(capi.Rect(0, 0, 1, 1)), C.byref(r)) == EINVAL
        assert L.ffhip_orient_inverse(o) == EINVAL
        with pytest.raises(capi.FfhipError):
            ops.orient_inverse(o)
    assert L.ffhip_orient_size(0, 3, 1, C.byref(w), C.byref(h)) == EINVAL and L.ffhip_orient_size(4, 0, 1, C.byref(w), C.byref(h)) == EINVAL
    assert L.ffhip_orient_size(4, 3, 1, None, C.byref(h)) == EINVAL and L.ffhip_orient_size(4, 3, 1, C.byref(w), None) == EINVAL
    assert L.ffhip_orient_rect(4, 3, 6, None, C.byref(r)) == EINVAL and L.ffhip_orient_rect(4, 3, 6, C.byref(capi.Rect(0, 0, 1, 1)), None) == EINVAL
    # the upright picture of a stored 4 x 3 is 3 x 4 under 6 and 4 x 3 under 3
    for o, bad in ((6, [(0, 0, 4, 3), (0, 0, 0, 1), (0, 0, 1, 0), (-1, 0, 1, 1), (0, -1, 1, 1), (3, 0, 1, 1), (0, 4, 1, 1), (1, 0, 3, 1), (0, 0, 2 ** 31 - 1, 1)]),
                   (3, [(0, 0, 3, 4), (0, 0, 5, 1), (4, 0, 1, 1), (0, 3, 1, 1), (2, 2, 2, 2)])):
        for rect in bad:
            assert lib_rect(L, 4, 3, o, rect)[0] == EINVAL, (o, rect)
    assert lib_rect(L, 4, 3, 6, (0, 0, 3, 4))[0] == 0 and lib_rect(L, 4, 3, 3, (0, 0, 4, 3))[0] == 0


# ---------------------------------------------------------------------------------------------------- refusals without a device
def item(**kw):
    """a good item: a 20 x 10 rectangle at (2, 3) of a picture with pitch 128, turned by 6 into a 10 x 20 picture with pitch 40"""
    it = capi.OrientItem()
    it.d_src, it.src_pitch, it.x0, it.y0, it.width, it.height = 0x10000, 128, 2, 3, 20, 10
    it.d_dst, it.dst_pitch, it.orientation = 0x20000, 40, 6
    for k, v in kw.items():
        setattr(it, k, v)
    return it


def call(L, items, n=None):
    arr = (capi.OrientItem * max(len(items), 1))(*items)
    return L.ffhip_bgra_orient_items(arr, len(items) if n is None else n, None)


BAD_ITEMS = {
    "orientation 0": dict(orientation=0), "orientation 9": dict(orientation=9), "orientation -1": dict(orientation=-1),
    "width 0": dict(width=0), "height 0": dict(height=0), "width -1": dict(width=-1), "x0 -1": dict(x0=-1), "y0 -1": dict(y0=-1),
    "no source": dict(d_src=None), "source at 2": dict(d_src=0x10002), "source at 1": dict(d_src=0x10001), "source pitch % 4": dict(src_pitch=130),
    "source pitch 0": dict(src_pitch=0), "rectangle wider than the pitch": dict(src_pitch=84),
    "rows past 31 bits": dict(src_pitch=1 << 20, y0=2040, height=9, dst_pitch=36), "y0 past 31 bits": dict(src_pitch=1 << 20, y0=0x7fffffff),
    "no destination": dict(d_dst=None), "destination at 1": dict(d_dst=0x20001), "destination at 2": dict(d_dst=0x20002),
    "destination pitch % 4": dict(dst_pitch=42), "destination pitch below the upright row": dict(dst_pitch=36),
    "destination pitch for the stored width under 3": dict(orientation=3, dst_pitch=76),
    "destination pitch for the stored row under 6, upright wider": dict(width=10, height=20, dst_pitch=40),
    "negative destination pitch": dict(dst_pitch=-40), "destination pitch past 2^32": dict(dst_pitch=(1 << 32) + 4),
}


@pytest.mark.parametrize("name", list(BAD_ITEMS))
def test_bad_items_are_refused_before_the_device_is_asked_for(L, name):
    for items in ([item(**BAD_ITEMS[name])], [item(), item(orientation=2, dst_pitch=80), item(**BAD_ITEMS[name])]):
        assert call(L, items) == EINVAL, name


def test_no_items_is_ok_and_bad_counts_are_refused(L):
    assert call(L, []) == 0 and L.ffhip_bgra_orient_items(None, 0, None) == 0
    assert call(L, [], n=-1) == EINVAL and L.ffhip_bgra_orient_items(None, 1, None) == EINVAL
    tensors.orient_bgra([])


def test_good_items_miss_the_device(L):
    if L.ffhip_device_count() > 0:
        pytest.skip("a GPU is present: these addresses are not memory; the -m gpu tests run the call")
    good = [item(), item(dst_pitch=1 << 32)] + [item(orientation=o, dst_pitch=80 if o < 5 else 40) for o in range(1, 9)]
    good += [item(width=1, height=1, dst_pitch=4, orientation=o) for o in (1, 6)] + [item(src_pitch=1 << 20, y0=2037, height=10)]
    for it in good:
        assert call(L, [it]) == ENODEV
    assert call(L, good) == ENODEV
    with pytest.raises(capi.FfhipError):
        tensors.orient_bgra([item()])


def file_call(L, entry, files, lens, n, fmt, outs, roi, size, filt, orient, orient_out, status, denom=None):
    if "jpeg" in entry:
        return getattr(L, entry)(files, lens, n, 2, fmt, outs, roi, size, filt, denom, None, orient, orient_out, None, status, None)
    return getattr(L, entry)(files, lens, n, 2, fmt, outs, roi, size, filt, orient, orient_out, None, status, None)


@pytest.mark.parametrize("entry", ["ffhip_jpeg_decode_files_tensor_oriented", "ffhip_webp_decode_files_tensor_oriented"])
def test_file_calls_refuse_bad_arguments_before_the_device(L, entry, jpeg, webp):
    data = np.frombuffer(X.tagged_jpeg(jpeg, 6) if "jpeg" in entry else X.tagged_webp(webp, 6), dtype=np.uint8)
    files, lens = (C.c_void_p * 2)(data.ctypes.data, data.ctypes.data), (C.c_size_t * 2)(data.size, data.size)
    outs, status, size = (capi.TensorOut * 2)(), (C.c_int * 2)(), (capi.Size * 2)(capi.Size(8, 8), capi.Size(8, 8))
    used = (C.c_int * 2)(-1, -1)
    f = tensors.tensor_format("uint8", "CHW", "RGB")
    bad = capi.TensorFormat()
    bad.dtype = 7
    turn = lambda *v: (C.c_int * 2)(*v)
    args = lambda **kw: {**dict(files=files, lens=lens, n=2, fmt=C.byref(f), outs=outs, roi=None, size=size, filt=AA, orient=None, orient_out=used,
                                status=status), **kw}
    assert file_call(L, entry, **args(n=0)) == 0
    assert file_call(L, entry, **args(files=None, lens=None, n=0, outs=None, size=None, status=None, orient_out=None)) == 0
    for kw in (dict(n=-1), dict(orient=turn(9, 1)), dict(orient=turn(1, 9)), dict(orient=turn(0, -1)), dict(orient=turn(6, 256 + 6)),
               dict(filt=2), dict(filt=-1, size=None), dict(fmt=None), dict(fmt=C.byref(bad)), dict(outs=None), dict(files=None), dict(lens=None),
               dict(status=None)):
        assert file_call(L, entry, **args(**kw)) == EINVAL, kw
        assert list(used) == [-1, -1]                                               # nothing was looked at
    if "jpeg" in entry:
        assert file_call(L, entry, **args(denom=turn(3, 1))) == EINVAL
        assert file_call(L, entry, **args(denom=turn(0, 1), size=None)) == EINVAL     # "choose" needs a size
    if L.ffhip_device_count() == 0:   # good arguments: the files are looked at, then the device is missed
        for kw in (dict(), dict(size=None), dict(orient=turn(0, 8)), dict(orient=turn(1, 1)), dict(orient_out=None)):
            assert file_call(L, entry, **args(**kw)) == ENODEV, kw
        assert file_call(L, entry, **args(orient=turn(0, 8))) == ENODEV and list(used) == [6, 8] and list(status) == [0, 0]
        assert file_call(L, entry, **args()) == ENODEV and list(used) == [6, 6]
        if "jpeg" in entry:
            assert file_call(L, entry, **args(denom=turn(0, 2))) == ENODEV
        # a file the probe refuses: orient_out 0
        junk = np.frombuffer(b"\xff\xd8 not a picture", dtype=np.uint8)
        files2, lens2 = (C.c_void_p * 2)(junk.ctypes.data, data.ctypes.data), (C.c_size_t * 2)(junk.size, data.size)
        assert file_call(L, entry, **args(files=files2, lens=lens2)) == ENODEV and list(used) == [0, 6] and status[0] != 0 and status[1] == 0


def test_python_argument_errors_come_before_the_device():
    files = [b"\xff\xd8 not a picture"] * 2
    for decode in (tensors.decode_jpeg_to_tensors, tensors.decode_webp_to_tensors):
        for orientation in (0, 9, True, [6], [6, 6, 6], [6, 0], "6"):
            with pytest.raises(ValueError):
                decode(files, orientation=orientation)


# ---------------------------------------------------------------------------------------------------- against PIL
@pytest.mark.parametrize("fmt", ["JPEG", "WEBP"])
def test_tag_and_upright_size_against_pil(L, fmt):
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    yy, xx = np.mgrid[0:31, 0:52]
    img = Image.fromarray(np.stack([xx * 4 % 256, yy * 8 % 256, (xx + yy) * 3 % 256], axis=2).astype(np.uint8))
    for o in range(1, 9):
        exif = Image.Exif()
        exif[0x0112] = o
        bio = io.BytesIO()
        img.save(bio, fmt, exif=exif, quality=80)
        data = bio.getvalue()
        assert read(L, data, webp=fmt == "WEBP") == (0, o)
        opened = Image.open(io.BytesIO(data))
        assert opened.getexif().get(0x0112) == o
        upright = ImageOps.exif_transpose(opened)
        assert ops.orient_size(52, 31, o) == upright.size
        # and the table: PIL's transpose of the decoded pixels is ours
        assert np.array_equal(np.asarray(upright), X.orient(np.asarray(opened), o))
