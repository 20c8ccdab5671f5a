#!/usr/bin/env python3
"""End-to-end throughput of the host codec pipeline (flyimg_amd/codec.py):
JPEG 1920x1080 q90 in -> decode (threads) -> GPU w_500,smc_1 -> JPEG q90 out,
batches of --batch images, first serially (decode, fi_process_batch with
pageable buffers, encode), then pipelined (CodecPipeline.process_batches:
decode into pinned slots, fi_submit_batch, encode of batch k during batch
k+1), then with the JPEGs decoded on the GPU (CodecPipeline gpu_decode).
Prints one JSON line with the stage splits; gpu_path_share = host time
blocked on the GPU path / wall.

--gpu-encode adds the A/B of the encode stage: the gpu_decode pipeline with
the outputs encoded by the host threads against the same pipeline with
gpu_encode (fi_jpeg_encode_device), --reps alternating passes over the same
batches after a warm-up pass of each: images/s and the host seconds in the
encode stage (median, min, max over the passes), the bytes a batch's outputs
are as pixels and as files (with gpu_encode the files are what crosses PCIe),
the size of the restart-marker files against the host encoder's files of the
same pixels, and -- from one more, event-timed pass -- the three encode
kernels' fi_kernel_stats times.

--progressive-encode is the A/B of CodecPipeline(gpu_progressive_encode=...)
alone: the gpu_decode pipeline with its outputs written as baseline files by
the GPU (gpu_encode), as progressive files with optimal tables by the GPU
(gpu_progressive_encode), and as progressive files by the host threads
(Pillow progressive=True), --reps alternating passes after a warm-up pass of
each: images/s, the host seconds in the encode stage, the bytes per batch, the
size of the progressive files against the restart-row baseline files of the
same pixels, the kernels' fi_kernel_stats times from one event-timed pass, and
--sweep: the two progressive arms at one batch of each listed size per pass.

--oriented is the A/B of CodecPipeline(gpu_orient=...) alone: the same sources
with an orientation-6 EXIF segment spliced in, --reps alternating passes with
the switch off (the host threads decode and rotate them) and on (they join
the GPU decode batch through fi_jpeg_decode_device_view), and -- from
event-timed passes -- k_jpeg_color_view on these files beside k_jpeg_color on
the same files without the segment.

--gpu-png is the A/B of CodecPipeline(gpu_png=...) alone: RGBA PNG sources
(seeded synth pictures plus an alpha ramp), w_500, --reps alternating passes
with the outputs written by the host threads' PNG writer and by
fi_png_encode_device after a warm-up pass of each: images/s, the host seconds
in the encode stage, the bytes over PCIe per batch, the five kernels'
fi_kernel_stats times from one more event-timed pass, and the sizes -- the GPU
files against Pillow's default and compress_level=1 files of the same pixels,
their IDAT payloads against zlib levels 1 and 6 on the same filtered stream.

--gpu-webp compares three ways out for --gpu-png's workload with
o_webp,webpl_1 appended, in --reps alternating passes after a warm-up pass of
each: gpu_png (the option ignored, the GPU PNG files), gpu_webp
(fi_webp_encode_device) and host_webp (the pixels downloaded, --threads
threads of Pillow save("WEBP", lossless=True, method=0)): images/s, the host
seconds in the encode stage, the five kernels' times from one more event-timed
pass, and the GPU WebP files' bytes against libwebp method 0 / 4 / 6 and
against the GPU PNG files of the same pixels.

--gpu-png-decode is the A/B of CodecPipeline(gpu_png_decode=...) on the same
RGBA PNG sources and request: --reps alternating passes, after a warm-up pass
of each, of the host-decode arm with gpu_png (the best arm before the device
decoder), of the device decoder with the host PNG writer, and of the fully
device-resident arm (gpu_png_decode + gpu_encode + gpu_png); the decode
kernels' fi_kernel_stats times from --reps event-timed passes; and --sweep, a
list of batch sizes at which the first and the last arm run one batch per pass
(an image's inflate is one wave: where the device decoder overtakes --threads
host threads is a matter of the batch)."""
import argparse
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--options", default="w_500,smc_1,q_90")
    ap.add_argument("--gpu-encode", action="store_true", help="A/B the encode stage: host threads against the GPU")
    ap.add_argument("--reps", type=int, default=5, help="alternating passes per setting of the --gpu-encode A/B")
    ap.add_argument("--progressive", action="store_true",
                    help="only the A/B of CodecPipeline(gpu_progressive=...) on progressive sources")
    ap.add_argument("--oriented", action="store_true",
                    help="only the A/B of CodecPipeline(gpu_orient=...) on orientation-6 sources")
    ap.add_argument("--gpu-png", action="store_true",
                    help="only the A/B of CodecPipeline(gpu_png=...) on RGBA PNG sources")
    ap.add_argument("--gpu-webp", action="store_true",
                    help="only the three-arm comparison of CodecPipeline(gpu_webp=...) on RGBA PNG sources")
    ap.add_argument("--gpu-png-decode", action="store_true",
                    help="only the A/B of CodecPipeline(gpu_png_decode=...) on RGBA PNG sources")
    ap.add_argument("--progressive-encode", action="store_true",
                    help="only the A/B of CodecPipeline(gpu_progressive_encode=...): GPU baseline, GPU progressive "
                         "and host-thread progressive files")
    ap.add_argument("--sweep", default="16,64,256,1024",
                    help="batch sizes of the --gpu-png-decode / --progressive-encode crossover sweep")
    a = ap.parse_args()
    if a.progressive_encode:
        return progressive_encode_ab(a)
    if a.gpu_png_decode:
        return png_decode_ab(a)
    if a.gpu_webp:
        return webp_ab(a)
    if a.gpu_png:
        return png_ab(a)
    if a.progressive:
        return progressive_ab(a)
    if a.oriented:
        return oriented_ab(a)
    import numpy as np
    from PIL import Image

    from flyimg_amd import codec
    from flyimg_amd.runtime import Context
    from flyimg_amd.synth import synth_rgb

    blobs = []
    for i in range(8):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(1920, 1080, 100 + i)).save(b, "JPEG", quality=90)
        blobs.append(b.getvalue())
    ctx = Context(0)
    pipe = codec.CodecPipeline(ctx, a.threads, gpu_decode=False)
    pipe.process(blobs[:2], [a.options] * 2)  # warm
    t_dec = t_gpu = t_enc = 0.0
    t0 = time.perf_counter()
    done = 0
    while done < a.images:
        n = min(a.batch, a.images - done)
        batch = [blobs[(done + k) % len(blobs)] for k in range(n)]
        s0 = time.perf_counter()
        px = list(pipe.pool.map(codec.decode, batch))
        s1 = time.perf_counter()
        from flyimg_amd.processor import ImageProcessor, OptionsBag
        ops = [ImageProcessor(OptionsBag(a.options), 1920, 1080).to_op()] * n
        outs, recs, rc = ctx.process([np.ascontiguousarray(p) for p in px], ops)
        s2 = time.perf_counter()
        list(pipe.pool.map(lambda o: codec.encode(o, 90), outs))
        s3 = time.perf_counter()
        t_dec += s1 - s0
        t_gpu += s2 - s1
        t_enc += s3 - s2
        done += n
    el = time.perf_counter() - t0
    serial = {"images": done, "images_per_s": round(done / el, 1),
              "input_mpix_per_s": round(done * 1920 * 1080 / 1e6 / el, 1), "wall_s": round(el, 3),
              "s_decode": round(t_dec, 3), "s_gpu_host_path": round(t_gpu, 3), "s_encode": round(t_enc, 3),
              "gpu_path_share": round(t_gpu / el, 4)}
    # pipelined: decode of batch k+1 into pinned memory + async submit overlap
    # batch k's DMA / kernels; batch k is encoded while k+1 runs
    batches = []
    done = 0
    while done < a.images:
        n = min(a.batch, a.images - done)
        batches.append(([blobs[(done + k) % len(blobs)] for k in range(n)], [a.options] * n))
        done += n
    for _ in pipe.process_batches(batches[:2]):  # warm the pinned slots
        pass
    t0 = time.perf_counter()
    got = sum(len(enc) for enc, _ in pipe.process_batches(batches))
    el = time.perf_counter() - t0
    st = pipe.stats
    piped = {"images": got, "images_per_s": round(got / el, 1), "input_mpix_per_s": round(got * 1920 * 1080 / 1e6 / el, 1),
             "wall_s": round(el, 3), "s_decode": round(st["s_decode"], 3), "s_gpu_wait": round(st["s_gpu_wait"], 3),
             "s_encode": round(st["s_encode"], 3), "gpu_path_share": round(st["s_gpu_wait"] / el, 4)}
    # GPU decode: CodecPipeline.process decodes the (baseline YCbCr) JPEGs on
    # the MI355X into device memory (fi_jpeg_decode_device), one device batch,
    # host threads only encode the outputs
    gpipe = codec.CodecPipeline(ctx, a.threads, gpu_decode=True)
    gpipe.process(blobs[:2], [a.options] * 2)  # warm
    t0 = time.perf_counter()
    done = 0
    while done < a.images:
        n = min(a.batch, a.images - done)
        gpipe.process([blobs[(done + k) % len(blobs)] for k in range(n)], [a.options] * n)
        done += n
    el = time.perf_counter() - t0
    gdec = {"images": done, "images_per_s": round(done / el, 1),
            "input_mpix_per_s": round(done * 1920 * 1080 / 1e6 / el, 1), "wall_s": round(el, 3)}
    gpipe.close()
    res = {"batch": a.batch, "threads": a.threads, "options": a.options, "serial": serial,
           "pipelined": piped, "gpu_decode": gdec}
    if a.gpu_encode:
        res["gpu_encode_ab"] = encode_ab(ctx, codec, blobs, a)
    print(json.dumps(res))
    pipe.close()
    ctx.close()


def png_payload(blob):
    """(IDAT payload, filtered stream) of a PNG file."""
    import struct
    import zlib

    pos, payload = 8, b""
    while pos < len(blob):
        n, typ = struct.unpack(">I4s", blob[pos:pos + 8])
        if typ == b"IDAT":
            payload += blob[pos + 8:pos + 8 + n]
        pos += 12 + n
    return payload, zlib.decompress(payload)


def png_sizes(gpu_files, pixels):
    """Size ratios of the GPU encoder's files of ``pixels`` (summed over them)."""
    import zlib

    from PIL import Image

    tot = {"gpu_file": 0, "pillow_default": 0, "pillow_level1": 0, "gpu_idat": 0, "zlib1": 0, "zlib6": 0, "stream": 0}
    for f, px in zip(gpu_files, pixels):
        payload, stream = png_payload(f)
        for key, kw in (("pillow_default", {}), ("pillow_level1", {"compress_level": 1})):
            b = io.BytesIO()
            Image.fromarray(px).save(b, "PNG", **kw)
            tot[key] += len(b.getvalue())
        tot["gpu_file"] += len(f)
        tot["gpu_idat"] += len(payload)
        tot["zlib1"] += len(zlib.compress(stream, 1))
        tot["zlib6"] += len(zlib.compress(stream, 6))
        tot["stream"] += len(stream)
    return {"bytes": tot,
            "file_vs_pillow_default": round(tot["gpu_file"] / tot["pillow_default"], 4),
            "file_vs_pillow_level1": round(tot["gpu_file"] / tot["pillow_level1"], 4),
            "idat_vs_zlib1": round(tot["gpu_idat"] / tot["zlib1"], 4),
            "idat_vs_zlib6": round(tot["gpu_idat"] / tot["zlib6"], 4)}


def png_ab(a):
    import statistics

    import numpy as np
    from PIL import Image

    from flyimg_amd import codec
    from flyimg_amd.runtime import Context
    from flyimg_amd.synth import synth_rgb

    W, H = 1000, 750
    options = "w_500"
    alpha = ((np.arange(W)[None, :] + 2 * np.arange(H)[:, None]) * 255 // (W + 2 * H)).astype(np.uint8)
    blobs = []
    for i in range(8):
        b = io.BytesIO()
        Image.fromarray(np.dstack([synth_rgb(W, H, 300 + i), alpha])).save(b, "PNG", compress_level=1)
        blobs.append(b.getvalue())
    ctx = Context(0)

    def spread(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def one_pass(pipe):
        pipe.process_stats = {"s_encode": 0.0, "raw_bytes": 0, "encoded_bytes": 0}
        t0 = time.perf_counter()
        done, files = 0, None
        while done < a.images:
            n = min(a.batch, a.images - done)
            files, _ = pipe.process([blobs[(done + k) % len(blobs)] for k in range(n)], [options] * n)
            done += n
        return done / (time.perf_counter() - t0), dict(pipe.process_stats), files

    pipes = {"host": codec.CodecPipeline(ctx, a.threads),
             "gpu": codec.CodecPipeline(ctx, a.threads, gpu_encode=True, gpu_png=True)}
    runs = {k: [] for k in pipes}
    last = {}
    for p in pipes.values():  # warm-up: every shape, every scratch buffer at its size
        one_pass(p)
    for _ in range(a.reps):
        for k, p in pipes.items():
            ips, st, last[k] = one_pass(p)
            runs[k].append((ips, st))
    out = {"source": f"{W}x{H} RGBA PNG", "options": options, "batch": a.batch, "threads": a.threads,
           "images": a.images, "reps": a.reps}
    nb = (a.images + a.batch - 1) // a.batch
    for k in pipes:
        st = runs[k][-1][1]
        out[k + "_png"] = {"images_per_s": spread([r[0] for r in runs[k]]),
                           "s_encode": spread([r[1]["s_encode"] for r in runs[k]]),
                           "raw_bytes_per_batch": st["raw_bytes"] // nb,
                           "file_bytes_per_batch": st["encoded_bytes"] // nb}
    # host arm: the pixels come back and the host writes the files; GPU arm: the
    # host-decoded batch's pixels come back, go up again and the files come back
    out["pcie_bytes_per_batch"] = {"host_png_d2h_pixels": out["host_png"]["raw_bytes_per_batch"],
                                   "gpu_png_d2h_pixels_h2d_pixels_d2h_files":
                                       2 * out["gpu_png"]["raw_bytes_per_batch"] + out["gpu_png"]["file_bytes_per_batch"]}
    n8 = min(8, len(last["gpu"]))
    pixels = [codec.decode(f) for f in last["host"][:n8]]
    assert all(np.array_equal(codec.decode(g), p) for g, p in zip(last["gpu"][:n8], pixels))
    out["sizes"] = png_sizes(last["gpu"][:n8], pixels)
    ctx.set_timing(1)
    ctx.reset_stats()
    one_pass(pipes["gpu"])
    out["kernel_ms_per_pass"] = {}
    for name in ("k_png_filter", "k_png_lz", "k_png_codes", "k_png_emit", "k_png_pack"):
        ms, launches, _ = ctx.stats(name)
        out["kernel_ms_per_pass"][name] = {"ms": round(ms, 3), "launches": launches}
    ctx.set_timing(0)
    ctx.reset_stats()
    for p in pipes.values():
        p.close()
    ctx.close()
    print(json.dumps({"gpu_png_ab": out}))


def webp_ab(a):
    """--gpu-webp: --gpu-png's workload with o_webp,webpl_1 appended, three
    arms in alternating passes: gpu_png (the GPU PNG files, the option
    ignored), gpu_webp (fi_webp_encode_device) and host_webp, the host
    alternative: the pixels downloaded and written by ``threads`` threads of
    Pillow save("WEBP", lossless=True, method=0)."""
    import statistics

    import numpy as np
    from PIL import Image

    from flyimg_amd import codec
    from flyimg_amd.runtime import Context
    from flyimg_amd.synth import synth_rgb

    W, H = 1000, 750
    options = "w_500,o_webp,webpl_1"
    alpha = ((np.arange(W)[None, :] + 2 * np.arange(H)[:, None]) * 255 // (W + 2 * H)).astype(np.uint8)
    blobs = []
    for i in range(8):
        b = io.BytesIO()
        Image.fromarray(np.dstack([synth_rgb(W, H, 300 + i), alpha])).save(b, "PNG", compress_level=1)
        blobs.append(b.getvalue())
    ctx = Context(0)

    def spread(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def pillow_webp(px, method=0):
        b = io.BytesIO()
        Image.fromarray(px).save(b, "WEBP", lossless=True, method=method)
        return b.getvalue()

    host_encode = codec.encode

    def one_pass(name):
        pipe = pipes[name]
        pipe.process_stats = {"s_encode": 0.0, "raw_bytes": 0, "encoded_bytes": 0}
        codec.encode = (lambda px, q: pillow_webp(px)) if name == "host_webp" else host_encode
        try:
            t0 = time.perf_counter()
            done, files = 0, None
            while done < a.images:
                n = min(a.batch, a.images - done)
                files, _ = pipe.process([blobs[(done + k) % len(blobs)] for k in range(n)], [options] * n)
                done += n
            return done / (time.perf_counter() - t0), dict(pipe.process_stats), files
        finally:
            codec.encode = host_encode

    pipes = {"gpu_png": codec.CodecPipeline(ctx, a.threads, gpu_encode=True, gpu_png=True),
             "gpu_webp": codec.CodecPipeline(ctx, a.threads, gpu_encode=True, gpu_png=True, gpu_webp=True),
             "host_webp": codec.CodecPipeline(ctx, a.threads)}
    runs = {k: [] for k in pipes}
    last = {}
    for k in pipes:  # warm-up: every shape, every scratch buffer at its size
        one_pass(k)
    for _ in range(a.reps):
        for k in pipes:
            ips, st, last[k] = one_pass(k)
            runs[k].append((ips, st))
    out = {"source": f"{W}x{H} RGBA PNG", "options": options, "batch": a.batch, "threads": a.threads,
           "images": a.images, "reps": a.reps}
    nb = (a.images + a.batch - 1) // a.batch
    for k in pipes:
        st = runs[k][-1][1]
        out[k] = {"images_per_s": spread([r[0] for r in runs[k]]),
                  "s_encode": spread([r[1]["s_encode"] for r in runs[k]]),
                  "raw_bytes_per_batch": st["raw_bytes"] // nb, "file_bytes_per_batch": st["encoded_bytes"] // nb}
    n8 = min(8, len(last["gpu_webp"]))
    pixels = [codec.decode(f) for f in last["gpu_png"][:n8]]
    for g, hw, p in zip(last["gpu_webp"][:n8], last["host_webp"][:n8], pixels):
        assert g[:4] == b"RIFF" and np.array_equal(np.asarray(Image.open(io.BytesIO(g))), p)
        vis = p[..., 3] > 0  # (libwebp without exact=True rewrites the colour under alpha 0)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(hw)))[vis], p[vis])
    tot = {"gpu_webp": sum(len(f) for f in last["gpu_webp"][:n8]), "gpu_png": sum(len(f) for f in last["gpu_png"][:n8])}
    for m in (0, 4, 6):
        tot[f"libwebp_method{m}"] = sum(len(pillow_webp(p, m)) for p in pixels)
    out["sizes"] = {"bytes": tot, **{f"gpu_webp_vs_{k}": round(tot["gpu_webp"] / v, 4)
                                      for k, v in tot.items() if k != "gpu_webp"}}
    ctx.set_timing(1)
    ctx.reset_stats()
    one_pass("gpu_webp")
    out["kernel_ms_per_pass"] = {}
    for name in ("k_webp_pred", "k_webp_lz", "k_webp_codes", "k_webp_emit", "k_webp_pack"):
        ms, launches, _ = ctx.stats(name)
        out["kernel_ms_per_pass"][name] = {"ms": round(ms, 3), "launches": launches}
    ctx.set_timing(0)
    ctx.reset_stats()
    for p in pipes.values():
        p.close()
    ctx.close()
    print(json.dumps({"gpu_webp_ab": out}))


def png_decode_ab(a):
    import statistics

    import numpy as np
    from PIL import Image

    from flyimg_amd import codec
    from flyimg_amd.runtime import Context
    from flyimg_amd.synth import synth_rgb

    W, H = 1000, 750
    options = "w_500"
    alpha = ((np.arange(W)[None, :] + 2 * np.arange(H)[:, None]) * 255 // (W + 2 * H)).astype(np.uint8)
    blobs = []
    for i in range(8):  # (the sources of --gpu-png)
        b = io.BytesIO()
        Image.fromarray(np.dstack([synth_rgb(W, H, 300 + i), alpha])).save(b, "PNG", compress_level=1)
        blobs.append(b.getvalue())
    ctx = Context(0)

    def spread(v, nd=1):
        return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    def one_pass(pipe, images, batch):
        t0 = time.perf_counter()
        done, files = 0, None
        while done < images:
            n = min(batch, images - done)
            files, _ = pipe.process([blobs[(done + k) % len(blobs)] for k in range(n)], [options] * n)
            done += n
        return done / (time.perf_counter() - t0), files

    pipes = {"host_decode_gpu_png": codec.CodecPipeline(ctx, a.threads, gpu_encode=True, gpu_png=True),
             "gpu_decode_host_png": codec.CodecPipeline(ctx, a.threads, gpu_png_decode=True),
             "gpu_decode_gpu_png": codec.CodecPipeline(ctx, a.threads, gpu_encode=True, gpu_png=True,
                                                       gpu_png_decode=True)}
    runs, last = {k: [] for k in pipes}, {}
    for p in pipes.values():  # warm-up: every shape, every scratch buffer at its size
        one_pass(p, a.images, a.batch)
    for _ in range(a.reps):
        for k, p in pipes.items():
            ips, last[k] = one_pass(p, a.images, a.batch)
            runs[k].append(ips)
    out = {"source": f"{W}x{H} RGBA PNG (Pillow compress_level=1)", "source_bytes": sum(map(len, blobs)) // len(blobs),
           "options": options, "batch": a.batch, "threads": a.threads, "images": a.images, "reps": a.reps}
    for k in pipes:
        out[k] = {"images_per_s": spread(runs[k]), "decode_stats": dict(pipes[k].decode_stats)}
    n8 = min(8, a.batch)
    pixels = [codec.decode(f) for f in last["host_decode_gpu_png"][:n8]]
    out["same_pixels"] = all(np.array_equal(codec.decode(f), p)
                             for k in pipes for f, p in zip(last[k][:n8], pixels))
    # the decode kernels, event-timed: per pass of --images in batches of --batch
    ctx.set_timing(1)
    names = ("k_png_inflate", "k_png_adler", "k_png_unfilter")
    ms = {n: [] for n in names}
    launches = 0
    for _ in range(a.reps):
        ctx.reset_stats()
        one_pass(pipes["gpu_decode_gpu_png"], a.images, a.batch)
        for n in names:
            t, launches, _ = ctx.stats(n)
            ms[n].append(t)
    ctx.set_timing(0)
    ctx.reset_stats()
    out["kernel_ms_per_pass"] = {n: dict(spread(v, 3), launches=launches) for n, v in ms.items()}
    # the crossover: one batch of B images per pass
    sweep = {}
    for bs in [int(s) for s in a.sweep.split(",") if s]:
        arms = ("host_decode_gpu_png", "gpu_decode_gpu_png")
        r = {k: [] for k in arms}
        for k in arms:
            one_pass(pipes[k], bs, bs)
        for _ in range(a.reps):
            for k in arms:
                r[k].append(one_pass(pipes[k], bs, bs)[0])
        sweep[str(bs)] = {k: spread(v) for k, v in r.items()}
        sweep[str(bs)]["gpu_over_host"] = round(statistics.median(r[arms[1]]) / statistics.median(r[arms[0]]), 3)
    out["sweep_images_per_s"] = sweep
    for p in pipes.values():
        p.close()
    ctx.close()
    print(json.dumps({"gpu_png_decode_ab": out}))


def progressive_ab(a):
    """Progressive 1080p sources through CodecPipeline.process with the
    gpu_progressive switch off (16 host threads decode them) and on (they join
    the GPU decode batch): alternating passes, images/s of each."""
    import statistics

    from PIL import Image

    from flyimg_amd import codec
    from flyimg_amd.runtime import Context
    from flyimg_amd.synth import synth_rgb

    blobs = []
    for i in range(8):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(1920, 1080, 100 + i)).save(b, "JPEG", quality=90, subsampling=2, progressive=True)
        blobs.append(b.getvalue())
    ctx = Context(0)
    pipes = {"off": codec.CodecPipeline(ctx, a.threads), "on": codec.CodecPipeline(ctx, a.threads, gpu_progressive=True)}

    def one_pass(pipe):
        t0 = time.perf_counter()
        done, files = 0, None
        while done < a.images:
            n = min(a.batch, a.images - done)
            files, _ = pipe.process([blobs[(done + k) % len(blobs)] for k in range(n)], [a.options] * n)
            done += n
        return done / (time.perf_counter() - t0), files

    last, runs = {}, {k: [] for k in pipes}
    for p in pipes.values():
        one_pass(p)  # warm-up
    for _ in range(a.reps):
        for k, p in pipes.items():
            ips, last[k] = one_pass(p)
            runs[k].append(ips)
    res = {"images": a.images, "batch": a.batch, "threads": a.threads, "options": a.options, "reps": a.reps,
           "sources": "1920x1080 q90 4:2:0 progressive (Pillow)", "same_output_bytes": last["on"] == last["off"]}
    for k, v in runs.items():
        res["gpu_progressive_" + k] = {"images_per_s": {"median": round(statistics.median(v), 1),
                                                        "min": round(min(v), 1), "max": round(max(v), 1)}}
    print(json.dumps(res))
    for p in pipes.values():
        p.close()
    ctx.close()


def progressive_encode_ab(a):
    """The encode stage three ways on the bench workload (1080p baseline
    sources, gpu_decode): GPU baseline files, GPU progressive files, and the
    host threads writing Pillow's progressive files."""
    import statistics

    import numpy as np
    from PIL import Image

    from flyimg_amd import codec
    from flyimg_amd.runtime import Context
    from flyimg_amd.synth import synth_rgb

    blobs = []
    for i in range(8):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(1920, 1080, 100 + i)).save(b, "JPEG", quality=90)
        blobs.append(b.getvalue())
    ctx = Context(0)

    def host_progressive(pixels, quality=90):  # codec.encode's settings with progressive=True
        ch = pixels.shape[2] if pixels.ndim == 3 else 1
        if ch in (2, 4):
            return plain_encode(pixels, quality)
        buf = io.BytesIO()
        Image.fromarray(pixels, "L" if ch == 1 else "RGB").save(
            buf, "JPEG", quality=int(quality), subsampling=0 if int(quality) >= 90 else 2, progressive=True)
        return buf.getvalue()

    def spread(v, nd=4):
        return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}

    plain_encode = codec.encode

    def one_pass(key, images, batch):
        pipe = pipes[key]
        pipe.process_stats = {"s_encode": 0.0, "raw_bytes": 0, "encoded_bytes": 0}
        codec.encode = host_progressive if key == "host_progressive" else plain_encode
        try:
            t0 = time.perf_counter()
            done, files = 0, None
            while done < images:
                n = min(batch, images - done)
                files, _ = pipe.process([blobs[(done + k) % len(blobs)] for k in range(n)], [a.options] * n)
                done += n
            return done / (time.perf_counter() - t0), dict(pipe.process_stats), files
        finally:
            codec.encode = plain_encode

    pipes = {"gpu_baseline": codec.CodecPipeline(ctx, a.threads, gpu_encode=True),
             "gpu_progressive": codec.CodecPipeline(ctx, a.threads, gpu_encode=True, gpu_progressive_encode=True),
             "host_progressive": codec.CodecPipeline(ctx, a.threads)}
    runs, last = {k: [] for k in pipes}, {}
    for k in pipes:  # warm-up: every shape, every scratch buffer at its size
        one_pass(k, a.images, a.batch)
    for _ in range(a.reps):
        for k in pipes:
            ips, st, last[k] = one_pass(k, a.images, a.batch)
            runs[k].append((ips, st))
    out = {"sources": "1920x1080 q90 (Pillow)", "options": a.options, "batch": a.batch, "threads": a.threads,
           "images": a.images, "reps": a.reps}
    nb = (a.images + a.batch - 1) // a.batch
    for k in pipes:
        st = runs[k][-1][1]
        out[k] = {"images_per_s": spread([r[0] for r in runs[k]], 1),
                  "s_encode": spread([r[1]["s_encode"] for r in runs[k]]),
                  "file_bytes_per_batch": st["encoded_bytes"] // nb}
    out["same_pixels"] = all(np.array_equal(codec.decode(f), codec.decode(g))
                             for f, g in zip(last["gpu_progressive"][:8], last["gpu_baseline"][:8]))
    out["progressive_over_restart_row_baseline_bytes"] = round(
        sum(map(len, last["gpu_progressive"])) / sum(map(len, last["gpu_baseline"])), 4)
    out["gpu_over_host_progressive_bytes"] = round(
        sum(map(len, last["gpu_progressive"])) / sum(map(len, last["host_progressive"])), 4)
    ctx.set_timing(1)
    out["kernel_ms_per_pass"] = {}
    for key, names in (("gpu_progressive", ("k_jpeg_fdct", "k_jpeg_pstat", "k_jpeg_ptab", "k_jpeg_pcode", "k_jpeg_ppack")),
                       ("gpu_baseline", ("k_jpeg_fdct", "k_jpeg_henc", "k_jpeg_pack"))):
        ctx.reset_stats()
        one_pass(key, a.images, a.batch)
        out["kernel_ms_per_pass"][key] = {}
        for name in names:
            ms, launches, _ = ctx.stats(name)
            out["kernel_ms_per_pass"][key][name] = {"ms": round(ms, 3), "launches": launches}
    ctx.set_timing(0)
    ctx.reset_stats()
    sweep = {}
    for bs in [int(x) for x in a.sweep.split(",") if x]:
        arms = ("host_progressive", "gpu_progressive")
        r = {k: [] for k in arms}
        for k in arms:
            one_pass(k, bs, bs)
        for _ in range(a.reps):
            for k in arms:
                r[k].append(one_pass(k, bs, bs)[0])
        sweep[str(bs)] = {k: spread(v, 1) for k, v in r.items()}
        sweep[str(bs)]["gpu_over_host"] = round(statistics.median(r[arms[1]]) / statistics.median(r[arms[0]]), 3)
    out["sweep_images_per_s"] = sweep
    for p in pipes.values():
        p.close()
    ctx.close()
    print(json.dumps({"gpu_progressive_encode_ab": out}))


def oriented_ab(a):
    """Orientation-6 1080p sources through CodecPipeline.process with the
    gpu_orient switch off and on, alternating passes; then one event-timed
    pass of each colour kernel: k_jpeg_color_view on the rotated files
    (and on orientation-3 copies, the same kernel without its LDS phase),
    k_jpeg_color on the same files without the EXIF segment."""
    import statistics
    import struct

    from PIL import Image

    from flyimg_amd import codec
    from flyimg_amd.runtime import Context
    from flyimg_amd.synth import synth_rgb

    # APP1: "Exif\0\0" + little-endian TIFF, IFD0 = {0x0112 SHORT 1: 6}
    def app1(o):
        body = b"Exif\x00\x00II*\x00" + struct.pack("<LHHHLHHL", 8, 1, 0x0112, 3, 1, o, 0, 0)
        return b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body

    plain, rotated, flipped = [], [], []  # no EXIF; orientation 6 (through LDS); orientation 3 (same kernel, no LDS)
    for i in range(8):
        b = io.BytesIO()
        Image.fromarray(synth_rgb(1920, 1080, 100 + i)).save(b, "JPEG", quality=90)
        blob = b.getvalue()
        cut = 4 + struct.unpack(">H", blob[4:6])[0]  # after the JFIF APP0
        plain.append(blob)
        rotated.append(blob[:cut] + app1(6) + blob[cut:])
        flipped.append(blob[:cut] + app1(3) + blob[cut:])
    ctx = Context(0)
    pipes = {"off": codec.CodecPipeline(ctx, a.threads), "on": codec.CodecPipeline(ctx, a.threads, gpu_orient=True)}

    def one_pass(pipe, blobs):
        t0 = time.perf_counter()
        done, files = 0, None
        while done < a.images:
            n = min(a.batch, a.images - done)
            files, _ = pipe.process([blobs[(done + k) % len(blobs)] for k in range(n)], [a.options] * n)
            done += n
        return done / (time.perf_counter() - t0), files

    last, runs = {}, {k: [] for k in pipes}
    for p in pipes.values():
        one_pass(p, rotated)  # warm-up
    for _ in range(a.reps):
        for k, p in pipes.items():
            ips, last[k] = one_pass(p, rotated)
            runs[k].append(ips)
    res = {"images": a.images, "batch": a.batch, "threads": a.threads, "options": a.options, "reps": a.reps,
           "sources": "1920x1080 q90 4:2:0 (Pillow), EXIF orientation 6", "same_output_bytes": last["on"] == last["off"],
           "decode_stats_on": dict(pipes["on"].decode_stats), "decode_stats_off": dict(pipes["off"].decode_stats)}
    for k, v in runs.items():
        res["gpu_orient_" + k] = {"images_per_s": {"median": round(statistics.median(v), 1),
                                                   "min": round(min(v), 1), "max": round(max(v), 1)}}
    # the colour kernels, event-timed: a warm pass, then --reps timed passes of each
    ctx.set_timing(1)
    kern = {}
    for key, name, blobs in (("k_jpeg_color_view", "k_jpeg_color_view", rotated),
                             ("k_jpeg_color_view_orientation_3", "k_jpeg_color_view", flipped),
                             ("k_jpeg_color", "k_jpeg_color", plain)):
        one_pass(pipes["on"], blobs)
        ms = []
        for _ in range(a.reps):
            ctx.reset_stats()
            one_pass(pipes["on"], blobs)
            t, launches, _ = ctx.stats(name)
            ms.append(t)
        kern[key] = {"ms_per_pass": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3),
                                      "max": round(max(ms), 3)}, "launches_per_pass": launches}
    ctx.set_timing(0)
    ctx.reset_stats()
    res["kernel"] = kern
    # orientation 6 over orientation 3: what the transposing path (the LDS phase and its barrier) costs
    res["rotate_over_flip"] = round(kern["k_jpeg_color_view"]["ms_per_pass"]["median"] /
                                    max(kern["k_jpeg_color_view_orientation_3"]["ms_per_pass"]["median"], 1e-9), 3)
    res["view_over_plain"] = round(kern["k_jpeg_color_view"]["ms_per_pass"]["median"] /
                                   max(kern["k_jpeg_color"]["ms_per_pass"]["median"], 1e-9), 3)
    print(json.dumps(res))
    for p in pipes.values():
        p.close()
    ctx.close()


def encode_ab(ctx, codec, blobs, a):
    import statistics

    def spread(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    def one_pass(pipe):
        pipe.process_stats = {"s_encode": 0.0, "raw_bytes": 0, "encoded_bytes": 0}
        t0 = time.perf_counter()
        done, files = 0, None
        while done < a.images:
            n = min(a.batch, a.images - done)
            files, _ = pipe.process([blobs[(done + k) % len(blobs)] for k in range(n)], [a.options] * n)
            done += n
        return done / (time.perf_counter() - t0), dict(pipe.process_stats), files

    pipes = {"host": codec.CodecPipeline(ctx, a.threads, gpu_decode=True),
             "gpu": codec.CodecPipeline(ctx, a.threads, gpu_decode=True, gpu_encode=True)}
    runs = {k: [] for k in pipes}
    last = {}
    for k, p in pipes.items():  # warm-up: every shape, every scratch buffer at its size
        one_pass(p)
    for _ in range(a.reps):
        for k, p in pipes.items():
            ips, st, last[k] = one_pass(p)
            runs[k].append((ips, st))
    out = {"images": a.images, "reps": a.reps}
    nb = (a.images + a.batch - 1) // a.batch
    for k in pipes:
        st = runs[k][-1][1]
        out[k + "_encode"] = {"images_per_s": spread([r[0] for r in runs[k]]),
                              "s_encode": spread([r[1]["s_encode"] for r in runs[k]]),
                              "raw_bytes_per_batch": st["raw_bytes"] // nb,
                              "file_bytes_per_batch": st["encoded_bytes"] // nb}
    out["d2h_bytes_per_batch"] = {"host_encode_pixels": out["host_encode"]["raw_bytes_per_batch"],
                                  "gpu_encode_files": out["gpu_encode"]["file_bytes_per_batch"]}
    # same pixels, same tables: what one restart interval per MCU row costs in bytes
    out["restart_rows_size_ratio"] = round(sum(map(len, last["gpu"])) / sum(map(len, last["host"])), 4)
    ctx.set_timing(1)
    ctx.reset_stats()
    one_pass(pipes["gpu"])
    out["kernel_ms_per_pass"] = {}
    for name in ("k_jpeg_fdct", "k_jpeg_henc", "k_jpeg_pack"):
        ms, launches, _ = ctx.stats(name)
        out["kernel_ms_per_pass"][name] = {"ms": round(ms, 3), "launches": launches}
    ctx.set_timing(0)
    ctx.reset_stats()
    for p in pipes.values():
        p.close()
    return out


if __name__ == "__main__":
    main()
