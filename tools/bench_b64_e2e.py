"""End-to-end throughput of the input encodings through one engine on one GPU.

Per format - ``b64`` (--input-format b64, decoded in the batch step), ``b64-ingest`` (the same
records with --b64-ingest: batch CRCs and the decode in the GPU ingest), ``byte-text`` (integer-pixel JSON through the default
GPU ingest) and ``float-text`` (Java Float.toString JSON through the default GPU ingest, what
bench.py streams) - an embedded broker is preloaded with N one-image records (a set of distinct
records appended by reference) and one engine serves them to ``max_records``. The rate is
images / s between the completion of the first ``--warm`` records and of the last one, read from
the completing thread's own clock (Engine.last_wait). The formats alternate for ``--rounds``
rounds in one process.

This is NOT bench.py's methodology (no feeder keeping a bounded backlog, no steady-state check,
no latency phase): it compares the formats with each other on a drained backlog, nothing more.
One JSON line per run; ``--out`` appends them to a file.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from gale._native import native  # noqa: E402
from gale.config import GaleConfig  # noqa: E402
from gale.data import (encode_batches, encode_records, encode_records_b64,  # noqa: E402
                       encode_records_text, preload, synthetic_pixels)
from gale.engine import Engine  # noqa: E402
from gale.models import get_model  # noqa: E402

K = native().kafka
CIFAR = dict(input_mean="0.4914,0.4822,0.4465", input_std="0.2470,0.2435,0.2616")


def records_for(fmt, pixels):
    if fmt in ("b64", "b64-ingest"):
        return encode_records_b64(pixels, 1)
    if fmt == "byte-text":
        return encode_records_text(pixels, 1)
    return encode_records((pixels.astype(np.float32) / np.float32(255.0)), 1)


def mark(eng):
    """(ns, records) of the completion that reached the last wait_completed target."""
    ns, c = eng.last_wait()
    if ns > 0:
        return ns, c
    return time.clock_gettime_ns(time.CLOCK_MONOTONIC), eng.completed  # (reached before the wait)


def run(fmt, a, pixels, rnd):
    net = get_model(a.model)
    recs = records_for(fmt, pixels)
    batches = encode_batches(recs, a.records_per_batch)
    broker = K.Broker(max_message_bytes=256 << 20)
    broker.start()
    try:
        broker.create_topic("in", a.partitions)
        broker.create_topic("out", 1)
        per_part = -(-a.records // a.partitions)
        total = 0
        for p in range(a.partitions):
            total += preload(broker, "in", p, batches, per_part, a.records_per_batch)[1]
        # the same model input for every format: pixels / 255, then the CIFAR mean / std
        prep = dict(CIFAR) if net.input_shape[2] == 3 else {}
        if fmt != "float-text":
            prep["input_scale"] = 1 / 255
        cfg = GaleConfig(topology_name=f"e2e-{fmt}", input_topic="in", output_topic="out",
                         bootstrap=f"127.0.0.1:{broker.port}", start_offset="earliest",
                         model=a.model, max_batch=a.batch, max_wait_us=2000,
                         queue_depth=4 * a.batch, source_parallelism=a.partitions,
                         sink_parallelism=2, replicas=a.replicas, decode_threads=a.decode_threads,
                         input_format="b64" if fmt in ("b64", "b64-ingest") else "json",
                         b64_ingest=fmt == "b64-ingest", stub=a.stub,
                         **prep).validate()
        eng = Engine(cfg, devices=None if a.stub else [0], max_records=total)
        eng.start()
        ok = eng.wait_completed(a.warm, a.timeout)
        t0, c0 = mark(eng)
        ok = ok and eng.wait_completed(total, a.timeout)
        t1, c1 = mark(eng)
        st = eng.stats()
        eng.stop()
    finally:
        broker.stop()
    if not ok or t1 <= t0:
        raise SystemExit(f"{fmt}: timed out ({st})")
    return dict(tool="bench_b64_e2e", format=fmt, round=rnd, model=a.model, records=total,
                warm_records=int(c0), timed_records=int(c1 - c0),
                timed_s=round((t1 - t0) * 1e-9, 4),
                img_s=round((c1 - c0) / ((t1 - t0) * 1e-9)),
                bytes_per_image=round(sum(len(r) for r in recs) / len(recs), 1),
                errors=int(st["errors"]), b64_records=int(st["b64_records"]),
                ingested_records=int(st["ingested_records"]),
                ingest_parsed_records=int(st.get("ingest_parsed_records", 0)),
                table_batches=int(st.get("table_batches", 0)), batch=a.batch,
                partitions=a.partitions, replicas=a.replicas, decode_threads=a.decode_threads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet20")
    ap.add_argument("--records", type=int, default=600000, help="records (= images) per run")
    ap.add_argument("--warm", type=int, default=200000, help="records before the timed part")
    ap.add_argument("--distinct", type=int, default=1024)
    ap.add_argument("--records-per-batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--formats", default="b64,b64-ingest,byte-text,float-text")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--partitions", type=int, default=11)
    ap.add_argument("--replicas", type=int, default=6)
    ap.add_argument("--decode-threads", type=int, default=12)
    ap.add_argument("--timeout", type=float, default=120.0)
    ap.add_argument("--stub", action="store_true", help="CPU stub replicas (the host path alone)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.warm >= a.records:
        ap.error("--warm must be below --records")
    pixels = synthetic_pixels(a.distinct, get_model(a.model).input_shape, 0)
    for rnd in range(a.rounds):
        for fmt in a.formats.split(","):
            line = json.dumps(run(fmt, a, pixels, rnd))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
