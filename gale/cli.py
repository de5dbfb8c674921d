"""``python -m gale`` — the MainTopology command line (R1) plus operational subcommands.

    python -m gale <TOPOLOGY_NAME> <INPUT_TOPIC> <OUTPUT_TOPIC> [--bootstrap H:P] [options]
        Run a topology (the reference's ``storm jar ... dke.model.MainTopology NAME IN OUT``,
        README.md:54-58, MainTopology.java:32-42). Unlike the reference, the Kafka address is a
        flag (the reference hard-codes empty zkHosts/bootstrap strings, :33-34) and every
        parallelism constant of :25-28 is an option. Runs for --duration seconds (reference: 1 h)
        or until ``python -m gale kill NAME`` / SIGTERM.
    python -m gale kill <NAME> [--wait-secs S]   (KillOptions wait_secs, :73-77)
    python -m gale list
    python -m gale broker [--port 9092] [--partitions N]     embedded Kafka-protocol broker
    python -m gale produce <TOPIC> [--images N] [--model M] [--rate R]   synthetic InstObj load
        [--pixels unit|byte] [--layout nhwc|nchw]     raw integer pixels / NCHW-nested records
        [--encoding json|b64]                         b64: base64 uint8 records (--pixels byte)
        [--size H,W]                                  images of that size (--input-size H,W)
        [--pixel-format rgb|i420|nv12|bgr24|rgba|bgra|gray]
                                                      YUV 4:2:0 frames / packed pixels
                                                      (--encoding b64; --input-pixel-format)
    python -m gale consume <TOPIC> [--max N] [--from-beginning]          print output records

``--profile DIR`` re-runs the topology under ``rocprofv3 --kernel-trace --marker-trace --stats``
(roctx ranges on every host pipeline stage, ``--trace``); ``GALE_ROCTX=1`` turns the ranges on
for an externally launched profiler.

Multi-GPU, one process per GPU: ``python -m gale NAME IN OUT --ranks 8`` starts and supervises
one rank process per GPU and respawns a rank that dies (Storm's supervisors, gale/supervisor.py);
``python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m gale NAME IN OUT
...`` runs the same ranks without respawning. Rank r consumes the input partitions
p % WORLD_SIZE == r (or its consumer-group share) and weights are RCCL-broadcast from rank 0.
"""

from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time
from dataclasses import fields
from typing import List, Optional

from gale.config import CHOICES, HELP, GaleConfig, from_sources

SUBCOMMANDS = ("kill", "list", "broker", "produce", "consume")


def _topology_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        prog="python -m gale",
        description="Run a gale streaming-inference topology (Kafka -> CNN replicas -> Kafka).",
        epilog=f"subcommands: {', '.join(SUBCOMMANDS)} (python -m gale <subcommand> -h)")
    ap.add_argument("topology_name", metavar="TOPOLOGY_NAME")
    ap.add_argument("input_topic", metavar="INPUT_TOPIC")
    ap.add_argument("output_topic", metavar="OUTPUT_TOPIC")
    ap.add_argument("--config", help="TOML file ([gale] table); CLI > env GALE_* > TOML")
    skip = {"topology_name", "input_topic", "output_topic"}
    for f in fields(GaleConfig):
        if f.name in skip:
            continue
        flag = "--" + f.name.replace("_", "-")
        t = f.type if isinstance(f.type, str) else f.type.__name__
        if t == "bool":
            ap.add_argument(flag, action=argparse.BooleanOptionalAction, default=None)
        else:
            kw = dict(default=None, type={"int": int, "float": float}.get(t, str))
            if f.name in CHOICES:  # ("" = not given: not a value to type)
                kw["choices"] = tuple(c for c in CHOICES[f.name] if c)
            if f.name in HELP:
                kw["help"] = HELP[f.name]
            if f.name == "top_k":
                kw["metavar"] = "K"
            ap.add_argument(flag, **kw)
    return ap


def parse_topology_args(argv: List[str]) -> GaleConfig:
    ns = vars(_topology_parser().parse_args(argv))
    toml_path = ns.pop("config")
    return from_sources(cli=ns, toml_path=toml_path)


def profile_command(cfg: GaleConfig, argv: List[str]) -> List[str]:
    """The rocprofv3 command that re-runs this topology (minus --profile) with roctx ranges on.

    Kernel dispatches + roctx markers + per-kernel stats land in ``cfg.profile`` (a directory).
    The program runs as a CHILD of this (GPU-untouched) process, right after ``--``: rocprofv3
    initialises the GPU in the profiled process, so no launcher may sit in between.
    """
    rest: List[str] = []
    skip_next = False
    for i, tok in enumerate(argv):
        if skip_next:
            skip_next = False
            continue
        if tok == "--profile":
            skip_next = True
            continue
        if tok.startswith("--profile="):
            continue
        rest.append(tok)
    return ["rocprofv3", "--kernel-trace", "--marker-trace", "--stats", "-d", cfg.profile,
            "-o", cfg.topology_name, "--", sys.executable, "-m", "gale", *rest, "--trace"]


def cmd_run(argv: List[str]) -> int:
    from gale.topology import (AlreadyAliveError, InvalidTopologyError, RankFailedError,
                               run_topology)

    cfg = parse_topology_args(argv)
    if cfg.ranks > 0 and not os.environ.get("GALE_SUPERVISED"):
        # the supervisor: one child process per rank, respawned when it dies (never touches
        # a GPU itself; gale/supervisor.py)
        from gale.supervisor import run_supervised

        logging.basicConfig(level=getattr(logging, cfg.log_level.upper(), logging.INFO),
                            format="%(asctime)s %(name)s %(levelname)s %(message)s")
        return run_supervised(cfg, argv)
    if cfg.profile:
        import subprocess

        # one HW queue per HIP stream in the profiled child: rocprofv3's queue interception
        # crashed when several of the engine's streams shared a HW queue and submitted
        # concurrently (GPU_MAX_HW_QUEUES=4 default; profiles/archive/r3_e2e_kernel_stats_default.csv)
        env = dict(os.environ)
        env.setdefault("GPU_MAX_HW_QUEUES", "32")
        return subprocess.call(profile_command(cfg, argv), env=env)
    logging.basicConfig(level=getattr(logging, cfg.log_level.upper(), logging.INFO),
                        format="%(asctime)s %(name)s %(levelname)s %(message)s")
    try:
        final = run_topology(cfg)
    except AlreadyAliveError as e:  # MainTopology.java:79-80 logs and returns
        logging.getLogger("gale").error("%s", e)
        return 1
    except InvalidTopologyError as e:
        logging.getLogger("gale").error("invalid topology: %s", e)
        return 2
    except RankFailedError as e:  # replaced by the rank supervisor (--ranks)
        logging.getLogger("gale").error("%s", e)
        return 3
    print(json.dumps({k: v for k, v in final.items() if k != "final"}), file=sys.stderr)
    return 0


def cmd_kill(argv: List[str]) -> int:
    from gale.topology import NotAliveError, Registry

    ap = argparse.ArgumentParser(prog="python -m gale kill")
    ap.add_argument("name")
    ap.add_argument("--wait-secs", type=float, default=0.0)
    ap.add_argument("--registry-dir", default=GaleConfig().registry_dir)
    a = ap.parse_args(argv)
    try:
        Registry(a.registry_dir).kill(a.name, a.wait_secs)
    except NotAliveError as e:  # MainTopology.java:85-86
        print(str(e), file=sys.stderr)
        return 1
    return 0


def cmd_list(argv: List[str]) -> int:
    from gale.topology import Registry

    ap = argparse.ArgumentParser(prog="python -m gale list")
    ap.add_argument("--registry-dir", default=GaleConfig().registry_dir)
    a = ap.parse_args(argv)
    for rec in Registry(a.registry_dir).list():
        print(json.dumps(rec))
    return 0


def cmd_broker(argv: List[str]) -> int:
    from gale._native import native

    ap = argparse.ArgumentParser(prog="python -m gale broker")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=9092)
    ap.add_argument("--partitions", type=int, default=1)
    ap.add_argument("--topics", default="", help="comma-separated topics to pre-create")
    ap.add_argument("--max-message-bytes", type=int, default=256 << 20)
    ap.add_argument("--duration", type=float, default=0, help="seconds (0 = until Ctrl-C)")
    a = ap.parse_args(argv)
    b = native().kafka.Broker(host=a.host, port=a.port, default_partitions=a.partitions,
                              max_message_bytes=a.max_message_bytes)
    b.start()
    for t in filter(None, a.topics.split(",")):
        b.create_topic(t, a.partitions)
    print(json.dumps({"broker": f"{a.host}:{b.port}", "partitions": a.partitions}), flush=True)
    try:
        t0 = time.time()
        while a.duration <= 0 or time.time() - t0 < a.duration:
            time.sleep(0.5)
    except KeyboardInterrupt:
        pass
    finally:
        b.stop()
    return 0


def produce_shape(input_shape, size: str):
    """(H, W, C) of ``produce``'s images: the model's, or ``--size H,W`` with its channels."""
    from gale.models.preprocess import RESIZE_MAX, parse_size

    hw = parse_size(size, "--size")
    if not hw:
        return tuple(input_shape)
    if len(hw) != 2 or not all(1 <= v <= RESIZE_MAX for v in hw):
        raise ValueError(f"--size: expected H,W with 1 <= H, W <= {RESIZE_MAX}, got {size!r}")
    return (hw[0], hw[1], input_shape[2])


def cmd_produce(argv: List[str]) -> int:
    import numpy as np

    from gale._native import native
    from gale.data import (encode_records, encode_records_b64, encode_records_text,
                           encode_records_packed, encode_records_typed, encode_records_yuv,
                           synthetic_images, synthetic_pixels, synthetic_yuv_planes)
    from gale.models import get_model

    ap = argparse.ArgumentParser(prog="python -m gale produce")
    ap.add_argument("topic")
    ap.add_argument("--bootstrap", default="127.0.0.1:9092")
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--images-per-record", type=int, default=1)
    ap.add_argument("--model", default="resnet20", choices=CHOICES["model"])
    ap.add_argument("--rate", type=float, default=0, help="records/s (0 = as fast as possible)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pixels", default="unit", choices=("unit", "byte"),
                    help="unit: floats in [0, 1); byte: integers 0..255 without a decimal point "
                         "(serve them with --input-scale 0.00392156862745098)")
    ap.add_argument("--layout", default="nhwc", choices=CHOICES["input_layout"],
                    help="nesting of each record's instances array (nchw: --input-layout nchw)")
    ap.add_argument("--encoding", default="json", choices=CHOICES["input_format"],
                    help="b64: one {\"b64\": ...} object of base64 uint8 pixels per image "
                         "(--input-format b64); needs --pixels byte")
    ap.add_argument("--size", default="", metavar="H,W",
                    help="size of the synthetic images (default: the model's; serve them with "
                         "--input-size H,W)")
    ap.add_argument("--pixel-format", default="rgb", choices=CHOICES["input_pixel_format"],
                    help="i420 / nv12: synthetic YUV 4:2:0 frames of HS*WS*3/2 bytes (serve them "
                         "with --input-pixel-format); needs --encoding b64, the nhwc layout, a "
                         "3-channel model and even sizes; bgr24 / rgba / bgra / gray: the "
                         "synthetic pixels of rgb in that byte order (alpha random; gray: their "
                         "first channel alone); needs --encoding b64, the nhwc layout and a "
                         "3-channel model")
    ap.add_argument("--input-dtype", default="u8", choices=CHOICES["input_dtype"],
                    help="u16 / f16 / bf16 / f32: the synthetic pixels (--pixels byte: 0..255; "
                         "unit: floats in [0, 1), not for u16) rounded to that type, little-endian "
                         "(serve them with --input-dtype); needs --encoding b64 and --pixel-format "
                         "rgb")
    a = ap.parse_args(argv)
    typed = a.input_dtype != "u8"
    if typed and (a.encoding != "b64" or a.pixel_format != "rgb"):
        ap.error(f"--input-dtype {a.input_dtype} needs --encoding b64 and --pixel-format rgb")
    if typed and a.input_dtype == "u16" and a.pixels != "byte":
        ap.error("--input-dtype u16 carries integers: it needs --pixels byte")
    packed = a.pixel_format in ("bgr24", "rgba", "bgra", "gray")
    yuv = a.pixel_format != "rgb" and not packed
    if (yuv or packed) and a.encoding != "b64":
        ap.error(f"--pixel-format {a.pixel_format} needs --encoding b64")
    if yuv and a.layout != "nhwc":
        ap.error(f"--pixel-format {a.pixel_format} has its own plane order: no --layout nchw")
    if packed and a.layout != "nhwc":
        ap.error(f"--pixel-format {a.pixel_format} has its own byte order: no --layout nchw")
    if a.encoding == "b64" and a.pixels != "byte" and not yuv and not typed:
        ap.error("--encoding b64 carries uint8 pixels: it needs --pixels byte")
    net = get_model(a.model)
    try:
        shape = produce_shape(net.input_shape, a.size)
    except ValueError as e:
        ap.error(str(e))
    if yuv:
        if shape[2] != 3 or shape[0] % 2 or shape[1] % 2:
            ap.error(f"--pixel-format {a.pixel_format} needs 3 channels and even sizes, got "
                     f"{shape}")
        recs = encode_records_yuv(*synthetic_yuv_planes(a.images, shape[0], shape[1], a.seed),
                                  a.pixel_format, a.images_per_record)
    elif packed:
        if shape[2] != 3:
            ap.error(f"--pixel-format {a.pixel_format} needs a 3-channel model, got {shape}")
        px = synthetic_pixels(a.images, shape, a.seed)  # (what --pixel-format rgb sends)
        alpha = None
        if a.pixel_format == "gray":
            px = np.repeat(px[..., :1], 3, axis=-1)
        elif a.pixel_format != "bgr24":
            alpha = np.random.default_rng(a.seed + 1).integers(0, 256, px.shape[:3],
                                                               dtype=np.uint8)
        recs = encode_records_packed(px, a.pixel_format, a.images_per_record, alpha)
    elif typed:
        imgs = (synthetic_pixels if a.pixels == "byte" else synthetic_images)(
            a.images, shape, a.seed)
        recs = encode_records_typed(imgs, a.input_dtype, a.images_per_record, a.layout)
    elif a.encoding == "b64":
        recs = encode_records_b64(synthetic_pixels(a.images, shape, a.seed),
                                  a.images_per_record, a.layout)
    elif a.pixels == "unit" and a.layout == "nhwc":
        recs = encode_records(synthetic_images(a.images, shape, a.seed),
                              a.images_per_record)
    else:  # written by Python's compact json.dumps
        imgs = (synthetic_pixels if a.pixels == "byte" else synthetic_images)(
            a.images, shape, a.seed)
        recs = encode_records_text(imgs, a.images_per_record, a.layout)
    p = native().kafka.Producer(a.bootstrap, linger_ms=5, batch_size=1 << 20)
    t0 = time.time()
    for i, r in enumerate(recs):
        if a.rate > 0:
            delay = t0 + i / a.rate - time.time()
            if delay > 0:
                time.sleep(delay)
        p.send(a.topic, r)
    p.flush()
    print(json.dumps({"produced": len(recs), "seconds": round(time.time() - t0, 3),
                      **p.stats()}))
    p.close()
    return 0


def cmd_consume(argv: List[str]) -> int:
    from gale._native import native

    ap = argparse.ArgumentParser(prog="python -m gale consume")
    ap.add_argument("topic")
    ap.add_argument("--bootstrap", default="127.0.0.1:9092")
    ap.add_argument("--max", type=int, default=10)
    ap.add_argument("--from-beginning", action="store_true")
    ap.add_argument("--timeout", type=float, default=10.0)
    a = ap.parse_args(argv)
    c = native().kafka.Consumer(a.bootstrap, max_wait_ms=200)
    c.assign(a.topic, [])
    c.seek_to("earliest" if a.from_beginning else "latest")
    n = 0
    t0 = time.time()
    while n < a.max and time.time() - t0 < a.timeout:
        for r in c.poll():
            v = r["value"]
            print(json.dumps({"partition": r["partition"], "offset": r["offset"],
                              "value": None if v is None else v.decode("utf-8", "replace")}))
            n += 1
            if n >= a.max:
                break
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] in SUBCOMMANDS:
        return {"kill": cmd_kill, "list": cmd_list, "broker": cmd_broker,
                "produce": cmd_produce, "consume": cmd_consume}[argv[0]](argv[1:])
    return cmd_run(argv)
