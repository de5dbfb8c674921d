"""One configuration object for a gale topology.

The reference spreads its configuration over three layers: compiled-in constants
(``NUM_WORKERS=8, KAFKA_SPOUT_PARAL=2, INFERENCE_BOLT_PARAL=4, KAFKA_BOLT_PARAL=2``,
MainTopology.java:25-28), hard-coded ``zkHosts`` / ``bootstrap`` strings that must be edited in
source (:33-34, README.md:38) and three positional CLI args (:36-38). gale keeps the positional
``<TOPOLOGY_NAME> <INPUT_TOPIC> <OUTPUT_TOPIC>`` contract and turns every knob into a field with
precedence

    CLI flag  >  environment (GALE_<FIELD>)  >  TOML file (--config)  >  default.
"""

from __future__ import annotations

import dataclasses
import os
from dataclasses import dataclass, field, fields
from typing import Any, Dict, List, Optional

CHOICES = {
    "replica_priority": ("normal", "high"),
    "step_launch": ("graph", "direct"),
    "sink_mode": ("async", "sync", "fire-and-forget"),
    "start_offset": ("latest", "earliest", "committed"),
    "auto_offset_reset": ("latest", "earliest"),
    "delivery": ("auto", "at-most-once", "at-least-once"),
    "value_format": ("json", "json-string"),
    "on_error": ("null", "error-json", "drop"),
    "output_key": ("none", "input"),
    "float_format": ("jdk19", "java8"),
    "assignor": ("range", "roundrobin", "load-aware"),
    "compression": ("none", "gzip", "snappy", "lz4", "zstd"),
    # compute dtype of the GPU kernels (MFMA bf16 / OCP e4m3 fp8 serving plans; fp32 = the
    # reference-precision plan on the fp32 matrix core, every tensor binary32 like the
    # reference's TF graph, InferenceBolt.java:80-86); inputs and the softmax output are fp32
    "dtype": ("bf16", "fp8", "fp32"),
    "model": ("lenet5", "resnet20", "resnet50"),
    # nesting order of a record's instances array (the model's tensors stay NHWC)
    "input_layout": ("nhwc", "nchw"),
    # what a record's instances array holds: "json" nested number arrays, "b64" one
    # {"b64": "<base64 of H*W*C uint8 values>"} object per image, decoded on the GPU
    "input_format": ("json", "b64"),
    # what a b64 record's bytes are: interleaved RGB, or a YUV 4:2:0 video frame (I420: three
    # planes; NV12: a Y plane and an interleaved UV plane) converted to RGB on the GPU
    # (gale/models/preprocess.py YuvConvert), or packed pixels (bgr24 / rgba / bgra: the named
    # byte order, alpha ignored; gray: one byte a pixel, replicated) unpacked to RGB on the GPU
    # (PixelUnpack). The names are ffmpeg's pix_fmts
    "input_pixel_format": ("rgb", "i420", "nv12", "bgr24", "rgba", "bgra", "gray"),
    # the YUV formats' matrix and range; "" = not given (bt601, limited)
    "input_yuv_matrix": ("", "bt601", "bt709"),
    "input_yuv_range": ("", "limited", "full"),
    # the element type of an rgb b64 string (gale/models/preprocess.py ElemType): one uint8 a
    # value, or little-endian 16-bit / float elements converted exactly on the GPU
    "input_dtype": ("u8", "u16", "f16", "bf16", "f32"),
}

TOP_K_MAX = 64  # --top-k: one winner per lane of the selection kernel's wave

# --help text of options that need more than their name
HELP = {
    "top_k": "K > 0: each image's output is {\"classes\": [...], \"scores\": [...]} of its K best "
             "classes, descending by score (ties to the lower class), instead of the whole "
             "softmax row; 1 <= K <= min(classes, 64); 0 = off (default)",
    "input_size": "HS,WS: the size every image of a record arrives in (default: the model's H,W); "
                  "the images are resized on the GPU (bilinear, no antialiasing) to "
                  "--input-resize and centre-cropped to the model's H,W",
    "input_resize": "HR,WR or S: the size an image is resampled to before the centre crop to the "
                    "model's H,W; S follows torchvision Resize(S): the shorter side of HS,WS "
                    "becomes S, the longer int(S*long/short); default: the model's H,W (plain "
                    "resize, no crop); HR >= H and WR >= W (no padding)",
    "input_pixel_format": "i420 / nv12: every b64 string is a YUV 4:2:0 frame of HS*WS*3/2 bytes "
                          "(HS,WS even; the model must have 3 channels), converted to RGB on the "
                          "GPU; bgr24 / rgba / bgra / gray: every b64 string is HS*WS pixels of "
                          "3 / 4 / 4 / 1 bytes in that byte order (alpha ignored, gray "
                          "replicated; any HS,WS; a 3-channel model), unpacked to RGB on the GPU; "
                          "--input-mean / --input-std stay in R,G,B order; all of them need "
                          "--input-format b64 and the nhwc layout; rgb (default): interleaved RGB "
                          "bytes",
    "input_yuv_matrix": "bt601 (default) or bt709; only with a YUV --input-pixel-format",
    "input_yuv_range": "limited (default: Y 16..235, chroma 16..240) or full; only with a YUV "
                       "--input-pixel-format",
    "input_dtype": "the element type of every b64 string: u8 (default) one byte a value; u16 / f16 "
                   "/ bf16 / f32: HS*WS*C little-endian elements of 2 / 2 / 2 / 4 bytes, converted "
                   "exactly to float32 on the GPU before --input-scale / --input-mean / "
                   "--input-std; an Inf or NaN element makes its record bad_number; anything but "
                   "u8 needs --input-format b64 and --input-pixel-format rgb",
    "input_antialias": "resample with the antialiased (support-scaled triangle) filter of PIL / "
                       "torchvision antialias=True instead of two-tap bilinear; needs an active "
                       "--input-size / --input-resize and a downscale of at most 8x per axis",
}


@dataclass
class GaleConfig:
    # positional contract (MainTopology.java:36-38)
    topology_name: str = "gale"
    input_topic: str = ""
    output_topic: str = ""
    # Kafka (R4, R5; the reference's zkHosts/bootstrap strings, MainTopology.java:33-34)
    bootstrap: str = "127.0.0.1:9092"
    embedded_broker: bool = False      # run an in-process broker on the bootstrap address
    broker_partitions: int = 1         # partitions of auto-created topics (embedded broker)
    group_id: str = ""                 # default: the topology name
    partitions: str = ""               # comma-separated input partitions (empty = all)
    start_offset: str = "latest"       # reference: LatestTime + ignoreZkOffsets (:101-102)
    auto_offset_reset: str = "latest"  # start_offset=committed / group-managed partitions with no
                                       # committed offset start here (Kafka auto.offset.reset)
    commit_interval_ms: int = 2000
    fetch_min_bytes: int = 1           # Kafka fetch.min.bytes of the consumers (long-poll size)
    fetch_max_wait_ms: int = 20        # Kafka fetch.max.wait.ms
    recv_lowat_kb: int = -1            # consumers wake per this many KB of a large fetch
                                       # response (SO_RCVLOWAT per receive call); 0 = per segment,
                                       # -1 = the bounce window with the bounce receive, else 0
    fetch_max_kb: int = 16384          # Kafka fetch.max.bytes (per fetch response)
    partition_max_kb: int = 8192       # Kafka max.partition.fetch.bytes
    pinned_fetch_mb: int = 4096        # pinned fetch-buffer budget per GPU (x2 with text_pack);
                                       # when it is spent the sources wait for a free buffer
    # elastic data parallelism: every process of the group shares the input partitions through
    # Kafka consumer-group membership; dead members' partitions move to the survivors
    group_membership: bool = False
    session_timeout_ms: int = 6000
    rebalance_timeout_ms: int = 8000
    heartbeat_interval_ms: int = 500
    assignor: str = "range"            # range | roundrobin | load-aware (capacity-weighted,
                                       # sticky; a member lagging behind triggers a rebalance)
    lag_rebalance_records: int = 0     # load-aware trigger: own lag above this and growing for
                                       # 1 s (0 = 8 x max_batch x replicas)
    rebalance_cooldown_ms: int = 10000  # load-aware: at most one lag-triggered rebalance per
                                        # cooldown
    decode_threads: int = 2            # CRC32C + envelope-scan workers behind each consumer
    check_crcs: bool = True            # Kafka consumer check.crcs
    gpu_ingest: bool = True            # CRC32C + image counts of pinned fetch buffers on the GPU
                                       # (the host reads only Kafka framing; csrc/runtime/ingest.h)
    text_pack: bool = True             # GPU ingest: sources nibble-pack fetch bodies for the
                                       # PCIe link, expanded on the device (text_pack.h); needs
                                       # AVX-512 VBMI; for hosts with idle cores behind a
                                       # link-bound GPU (profiles/archive/r3_nibble_transport_ab.txt)
    text_pack_bounce: bool = True      # with text_pack: fetch bodies go through a cache-resident
                                       # window; the pinned chunk gets the packed text and a
                                       # sparse framing copy only (csrc/runtime/pack_tap.h)
    text_pack_window_kb: int = 256     # that window, per source thread
    ingest_parse: bool = True          # GPU ingest: parse each fetch's records into an fp32 image
                                       # arena right behind its counting launch, so the batch
                                       # step of a whole-network plan (LeNet-5, ResNet-20) runs
                                       # the forward only (images through a pointer table)
    # parallelism (R3)
    workers: int = 8                   # NUM_WORKERS: placement only (one process per GPU here)
    source_parallelism: int = 2        # KAFKA_SPOUT_PARAL
    replicas: int = 0                  # INFERENCE_BOLT_PARAL; 0 = one per visible GPU
    sink_parallelism: int = 2          # KAFKA_BOLT_PARAL
    gpus: int = 0                      # GPUs to use (0 = all visible)
    numa_pin: bool = True              # a process serving ONE GPU pins its threads to that
                                       # GPU's NUMA node (gale.utils.pin_to_gpu_numa)
    locality_split: int = 1            # locality slots per GPU (single process): K slots on one
                                       # device, each with its own sources, batcher, pinned
                                       # pool + device mirror; a slot's idle replicas steal from
                                       # the others and parse stolen text from host-pinned
                                       # memory, as across GPUs (the multi-GPU dispatch on 1 GPU)
    # sink (R9, E7-E9)
    acks: int = 1                      # MainTopology.java:113
    sink_mode: str = "async"           # KafkaBolt async / sync / fire-and-forget
    # delivery of outputs: at-most-once = the reference (a failed send fails the unanchored tuple,
    # nothing replays it, KafkaBolt.java:133-137); at-least-once = an output that is never
    # acknowledged keeps its input offset uncommitted and the rank exits non-zero to be respawned
    # from the committed offsets; auto = at-least-once when offsets are resumed (start_offset
    # committed or group membership), else at-most-once
    delivery: str = "auto"
    producer_retries: int = 3          # kafka-clients retries (0.11 default 0): retriable produce
                                       # errors are re-sent after retry_backoff_ms
    retry_backoff_ms: int = 100        # retry.backoff.ms
    delivery_timeout_ms: int = 120000  # delivery.timeout.ms: no retry after this long
    value_format: str = "json"         # json-string = spring JsonSerializer double encoding
    type_id_header: bool = False       # add __TypeId__: java.lang.String (spring JsonSerializer)
    linger_ms: int = 0
    compression: str = "none"          # sink compression.type: none | gzip | snappy | lz4 | zstd
                                       # (kafka-clients default none; the input side decodes
                                       # every codec and the old message formats regardless)
    on_error: str = "null"             # reference: malformed input -> null record
    output_key: str = "none"           # reference: unkeyed output (E9); "input" = input's key
    float_format: str = "jdk19"        # prediction digits: jdk19 = shortest round-trip (GPU
                                       # formatted); java8 = the reference runtime's
                                       # Float.toString (host formatted, csrc/codec/java8_float.cpp)
    top_k: int = 0                     # > 0: each image's output is {"classes": [...], "scores":
                                       # [...]} of its K best classes in score order instead of
                                       # the whole softmax row; 1 <= K <= min(classes, 64)
                                       # (selected on the GPU with gpu_encode: topk.hip)
    producer_buffer_mb: int = 32       # unsent output bytes per sink producer before the sink
                                       # blocks (Kafka buffer.memory, 32 MB default)
    producer_request_kb: int = 1024    # bytes per produce request (Kafka max.request.size)
    output_partition: int = -1         # -1: the producer's partitioner (reference: unkeyed
                                       # round-robin); >= 0: every output record to this
                                       # partition (e.g. the one this process's broker leads)
    # lifetime (reference: sleep 1 h then kill, MainTopology.java:71-77)
    duration: float = 3600.0
    # model / compute
    model: str = "resnet20"
    dtype: str = "bf16"
    weights: str = ""                  # .npz / .safetensors (torch layout); empty = seeded init
    seed: int = 0
    # input preprocessing, applied where the records are parsed (gale/models/preprocess.py):
    # model input = (x * input_scale - mean[c]) / std[c]; mean / std are comma-separated lists of
    # 1 value (broadcast) or one per channel (C <= 4), in the units after scaling
    input_scale: float = 1.0
    input_mean: str = ""
    input_std: str = ""
    input_layout: str = "nhwc"         # nchw: records nest [N][C][H][W]
    # input resize (gale/models/preprocess.py InputResize): records carry input_size images,
    # resized (bilinear, half-pixel centres, no antialiasing) to input_resize and centre-cropped
    # to the model's H,W after the preprocessing; both empty = off (model-size records)
    input_size: str = ""               # "HS,WS": the size every image of a record arrives in
    input_resize: str = ""             # "HR,WR" or "S" (torchvision Resize(S) on HS,WS)
    input_antialias: bool = False      # the antialiased tap filter on both axes (downscale <= 8x)
    input_format: str = "json"         # b64: base64 uint8 image records (no text packing; GPU
                                       # ingest only with b64_ingest)
    input_pixel_format: str = "rgb"    # i420 | nv12: b64 strings are YUV 4:2:0 frames;
                                       # bgr24 | rgba | bgra | gray: packed pixels
    input_yuv_matrix: str = ""         # bt601 (default) | bt709, YUV formats only
    input_yuv_range: str = ""          # limited (default) | full, YUV formats only
    input_dtype: str = "u8"            # u16 | f16 | bf16 | f32: rgb b64 strings carry little-endian
                                       # elements of that type (typed tensor records)
    b64_ingest: bool = False           # input_format b64: GPU ingest of each fetch (batch CRCs on
                                       # the device, strings decoded into the fetch's image
                                       # arena, the table step); needs gpu_ingest, no effect
                                       # with stub replicas
    max_batch: int = 256
    max_wait_us: int = 2000
    slo_p99_ms: float = 0.0            # latency-SLO mode (config 5): adapt batch/wait to a p99
    queue_depth: int = 8192
    use_graph: bool = True
    graph_step: bool = True            # whole-network plans: each batch step (metadata H2D,
                                       # parse, forward, format, status D2H) is ONE replay of a
                                       # per-slot captured hipGraph (else launched op by op)
    gpu_wait_poll_us: int = 20         # > 0: replicas sleep-poll their batch events (0: spin)
    step_launch: str = "direct"        # the kernels-only batch step (parse -> forward) launched
                                       # kernel by kernel ("direct") or as a hipGraph replay
                                       # ("graph": the runtime's graph-launch bookkeeping kept a
                                       # helper thread spinning at ~0.8 of a core,
                                       # profiles/r5_ab_step_launch.jsonl)
    replica_priority: str = "normal"   # high: replica streams at the top stream priority (their
                                       # step kernels dispatch ahead of the GPU ingest's)
    gpu_encode: bool = True            # prediction text (Float.toString) formatted on the GPU
    fold_bn: bool = True               # False: standalone BatchNorm kernels (bf16 / fp32)
    stub: bool = False                 # CPU stub replicas (plumbing without a GPU)
    stub_null: bool = False            # stub replicas skip parsing/compute (host-path benchmark)
    stub_delay_us: int = 0             # stub replicas: emulated device time per batch
    # robustness / observability
    watchdog_ms: int = 30000
    # supervisor (Storm supervisors restart dead workers): a replica that failed is
    # recovered and rejoins after restart_backoff_ms, up to max_restarts times (0 = stays dead)
    max_restarts: int = 3
    restart_backoff_ms: int = 500
    # rank supervisor (gale/supervisor.py; Storm supervisors respawn dead worker JVMs,
    # MainTopology.java:25,65-66): > 0 = this command starts and supervises that many rank
    # processes (one per GPU), respawning a dead one after rank_restart_backoff_ms, at most
    # rank_max_restarts times per rank (-1 = always)
    ranks: int = 0
    rank_max_restarts: int = 10
    rank_restart_backoff_ms: int = 1000
    rank_start_timeout_s: float = 300.0
    # more ranks than GPUs (a 1-GPU rehearsal of the multi-rank path): rank r serves GPU
    # r % device_count and the process group is gloo (RCCL refuses two ranks on one device)
    shared_gpu_rehearsal: bool = False
    fault: str = ""                    # replica_crash@N,parse_error@P,producer_fail@P
    trace: bool = False                # roctx ranges around pipeline stages (rocprofv3)
    profile: str = ""                  # run under rocprofv3 --kernel-trace --marker-trace --stats
    metrics_interval: float = 10.0
    metrics_file: str = ""             # JSON lines; empty = stderr
    metrics_port: int = -1             # >= 0: HTTP /metrics (Prometheus) + /stats (JSON) on
                                       # 127.0.0.1:port+local_rank (0 = any free port); -1 off
    log_level: str = "INFO"
    registry_dir: str = field(default_factory=lambda: os.path.join(
        os.path.expanduser("~"), ".gale", "topologies"))

    def validate(self) -> "GaleConfig":
        if self.producer_request_kb < 1:
            raise ValueError("--producer-request-kb must be >= 1")
        if self.producer_buffer_mb < 1:
            raise ValueError("--producer-buffer-mb must be >= 1")
        if self.output_partition < -1:
            raise ValueError("--output-partition must be -1 (partitioner) or a partition index")
        for k, allowed in CHOICES.items():
            v = getattr(self, k)
            if v not in allowed:
                raise ValueError(f"{k}={v!r}: expected one of {allowed}")
        if self.acks not in (0, 1, -1):
            raise ValueError("acks must be 0, 1 or -1")
        for k in ("source_parallelism", "sink_parallelism", "max_batch", "queue_depth"):
            if getattr(self, k) <= 0:
                raise ValueError(f"{k} must be positive")
        if self.group_membership and not (0 < self.heartbeat_interval_ms
                                          < self.session_timeout_ms):
            raise ValueError("group membership: need 0 < heartbeat_interval_ms < "
                             "session_timeout_ms")
        if self.slo_p99_ms < 0:
            raise ValueError("slo_p99_ms must be >= 0")
        if self.replicas < 0 or self.gpus < 0:
            raise ValueError("replicas/gpus must be >= 0")
        if self.ranks < 0 or self.rank_restart_backoff_ms < 0:
            raise ValueError("--ranks / --rank-restart-backoff-ms must be >= 0")
        if self.producer_retries < 0 or self.retry_backoff_ms < 0 or self.delivery_timeout_ms < 1:
            raise ValueError("--producer-retries / --retry-backoff-ms must be >= 0, "
                             "--delivery-timeout-ms >= 1")
        if self.effective_delivery == "at-least-once" and self.sink_mode == "fire-and-forget":
            raise ValueError("at-least-once delivery needs acknowledged sends: --sink-mode "
                             "async|sync (or --delivery at-most-once)")
        if self.locality_split < 1:
            raise ValueError("locality_split must be >= 1")
        if not self.topology_name:
            raise ValueError("topology name is required")
        if not self.fold_bn and self.dtype == "fp8":
            raise ValueError("--no-fold-bn (standalone BatchNorm plan) is bf16 / fp32 only")
        if self.b64_ingest and self.input_format != "b64":
            raise ValueError("--b64-ingest needs --input-format b64")
        self.input_prep()  # (ValueError on a bad scale / mean / std / layout)
        # (ValueError naming --input-size / --input-resize / --input-antialias)
        rs = self.input_resize_plan()
        self._validate_pixel_format(rs)
        self._validate_dtype()
        if self.top_k != 0:
            from gale.models import get_model

            classes = get_model(self.model).classes
            if not 1 <= self.top_k <= min(classes, TOP_K_MAX):
                raise ValueError(f"--top-k {self.top_k}: expected 0 (off) or 1 <= K <= "
                                 f"{min(classes, TOP_K_MAX)} (the smaller of {self.model}'s "
                                 f"{classes} classes and {TOP_K_MAX})")
        return self

    def _validate_pixel_format(self, rs) -> None:
        """ValueError naming the option for a YUV or packed pixel format that cannot be served."""
        fmt = self.input_pixel_format
        yuv = fmt in ("i420", "nv12")
        if not yuv:
            for k in ("input_yuv_matrix", "input_yuv_range"):
                if getattr(self, k):
                    raise ValueError(f"--{k.replace('_', '-')} applies to the YUV formats only: "
                                     "it needs --input-pixel-format i420 or nv12")
        if fmt == "rgb":
            return
        from gale.models import get_model

        if self.input_format != "b64":
            raise ValueError(f"--input-pixel-format {fmt} needs --input-format b64")
        if self.input_layout != "nhwc":
            raise ValueError(f"--input-pixel-format {fmt} has its own "
                             f"{'plane' if yuv else 'byte'} order: "
                             "--input-layout nchw does not apply")
        C = get_model(self.model).input_shape[2]
        if C != 3:
            hint = ("; --input-pixel-format rgb already carries one byte per pixel for a "
                    "1-channel model" if fmt == "gray" and C == 1 else "")
            raise ValueError(f"--input-pixel-format {fmt} gives 3-channel RGB; {self.model} "
                             f"takes C = {C}{hint}")
        if yuv and (rs.HS % 2 or rs.WS % 2):
            opt = "--input-size" if self.input_size else "--input-pixel-format"
            raise ValueError(f"{opt}: a 4:2:0 frame (--input-pixel-format {fmt}) needs even "
                             f"HS,WS, got {rs.HS},{rs.WS}")

    def _validate_dtype(self) -> None:
        """ValueError naming the option for an element type that cannot be served. (Per-channel
        coefficients with C > 4 are refused by input_prep(), by --input-mean / --input-std.)"""
        dt = self.input_dtype
        if dt == "u8":
            return
        if self.input_format != "b64":
            raise ValueError(f"--input-dtype {dt} needs --input-format b64")
        if self.input_pixel_format != "rgb":
            raise ValueError(f"--input-dtype {dt} names the elements of an rgb tensor: it needs "
                             f"--input-pixel-format rgb, not {self.input_pixel_format}")

    def input_elem(self):
        """The ``ElemType`` of this configuration, None for u8."""
        from gale.models.preprocess import ElemType

        return ElemType.from_config(self)

    def input_yuv(self):
        """The ``YuvConvert`` of this configuration, None for rgb."""
        from gale.models.preprocess import YuvConvert

        return YuvConvert.from_config(self)

    def input_unpack(self):
        """The ``PixelUnpack`` of this configuration, None for rgb and the YUV formats."""
        from gale.models.preprocess import PixelUnpack

        return PixelUnpack.from_config(self)

    def input_prep(self, C: Optional[int] = None):
        """The ``InputPrep`` of this configuration (C: the model's input channels)."""
        from gale.models.preprocess import InputPrep

        if C is None:
            from gale.models import get_model

            C = get_model(self.model).input_shape[2]
        return InputPrep.from_config(self, C)

    def input_resize_plan(self, H: Optional[int] = None, W: Optional[int] = None):
        """The ``InputResize`` of this configuration (H, W: the model's input size)."""
        from gale.models.preprocess import InputResize

        if H is None or W is None:
            from gale.models import get_model

            H, W = get_model(self.model).input_shape[:2]
        try:
            return InputResize.build(H, W, self.input_size, self.input_resize,
                                     self.input_antialias)
        except ValueError as e:
            raise ValueError("--" + str(e).replace("_", "-", 1)) from None

    @property
    def effective_group(self) -> str:
        return self.group_id or self.topology_name

    @property
    def effective_delivery(self) -> str:
        if self.delivery != "auto":
            return self.delivery
        resumes = self.start_offset == "committed" or self.group_membership
        return "at-least-once" if resumes and self.sink_mode != "fire-and-forget" \
            else "at-most-once"

    def engine_dict(self, H: int, W: int, C: int, classes: int) -> Dict[str, Any]:
        """Keyword dict for the native ``gale._C.Engine``."""
        return dict(
            bootstrap=self.bootstrap, input_topic=self.input_topic, output_topic=self.output_topic,
            group_id=self.effective_group, client_id=self.topology_name,
            partitions=[int(p) for p in self.partitions.split(",") if p.strip()],
            source_parallelism=self.source_parallelism, start_offset=self.start_offset,
            auto_offset_reset=self.auto_offset_reset, delivery=self.effective_delivery,
            producer_retries=self.producer_retries, retry_backoff_ms=self.retry_backoff_ms,
            delivery_timeout_ms=self.delivery_timeout_ms,
            commit_interval_ms=self.commit_interval_ms, sink_parallelism=self.sink_parallelism,
            fetch_min_bytes=self.fetch_min_bytes, fetch_max_wait_ms=self.fetch_max_wait_ms,
            recv_lowat=self.recv_lowat_kb << 10 if self.recv_lowat_kb >= 0 else -1,
            fetch_max_bytes=self.fetch_max_kb << 10,
            partition_max_bytes=self.partition_max_kb << 10,
            pinned_fetch_bytes=self.pinned_fetch_mb << 20,
            group_membership=self.group_membership, session_timeout_ms=self.session_timeout_ms,
            rebalance_timeout_ms=self.rebalance_timeout_ms,
            heartbeat_interval_ms=self.heartbeat_interval_ms, assignor=self.assignor,
            lag_rebalance_records=self.lag_rebalance_records,
            rebalance_cooldown_ms=self.rebalance_cooldown_ms,
            decode_threads=self.decode_threads, check_crcs=self.check_crcs,
            text_pack=bool(self.gpu_ingest and self.text_pack and self.input_format == "json"
                           and _pack_fast()),
            text_pack_bounce=self.text_pack_bounce, text_pack_window_kb=self.text_pack_window_kb,
            acks=self.acks, sink_mode=self.sink_mode, linger_ms=self.linger_ms,
            compression=self.compression,
            value_format=self.value_format, type_id_header=self.type_id_header,
            on_error=self.on_error, output_key=self.output_key, float_format=self.float_format,
            top_k=self.top_k, output_partition=self.output_partition,
            producer_buffer_bytes=self.producer_buffer_mb << 20,
            producer_request_bytes=self.producer_request_kb << 10, H=H, W=W, C=C, classes=classes,
            max_batch=self.max_batch,
            max_wait_us=self.max_wait_us, slo_p99_ms=self.slo_p99_ms,
            queue_depth=self.queue_depth,
            watchdog_ms=self.watchdog_ms, max_restarts=self.max_restarts,
            restart_backoff_ms=self.restart_backoff_ms, fault=self.fault, seed=self.seed,
            trace=self.trace, input_format=self.input_format, b64_ingest=self.b64_ingest,
            **self.input_prep(C).engine_entries(),
            **self.input_resize_plan(H, W).engine_entries(),
            **(self.input_yuv().engine_entries() if self.input_yuv() else {}),
            **(self.input_unpack().engine_entries() if self.input_unpack() else {}),
            **(self.input_elem().engine_entries() if self.input_elem() else {}))


def _pack_fast() -> bool:
    from gale._native import native

    return bool(native().text_pack_fast())


def _coerce(f: dataclasses.Field, raw: Any) -> Any:
    t = f.type if isinstance(f.type, str) else getattr(f.type, "__name__", str(f.type))
    if t == "bool":
        if isinstance(raw, bool):
            return raw
        s = str(raw).strip().lower()
        if s in ("1", "true", "yes", "on"):
            return True
        if s in ("0", "false", "no", "off", ""):
            return False
        raise ValueError(f"{f.name}: not a boolean: {raw!r}")
    if t == "int":
        return int(raw)
    if t == "float":
        return float(raw)
    return str(raw)


def from_sources(cli: Optional[Dict[str, Any]] = None, env: Optional[Dict[str, str]] = None,
                 toml_path: Optional[str] = None) -> GaleConfig:
    """Merge defaults < TOML < env (GALE_*) < CLI (only keys explicitly given)."""
    env = os.environ if env is None else env
    values: Dict[str, Any] = {}
    known = {f.name: f for f in fields(GaleConfig)}
    if toml_path:
        import tomli

        with open(toml_path, "rb") as fh:
            data = tomli.load(fh)
        data = data.get("gale", data)
        for k, v in data.items():
            k = k.replace("-", "_")
            if k not in known:
                raise ValueError(f"{toml_path}: unknown key {k!r}")
            values[k] = _coerce(known[k], v)
    for name, f in known.items():
        ev = env.get("GALE_" + name.upper())
        if ev is not None:
            values[name] = _coerce(f, ev)
    for k, v in (cli or {}).items():
        if v is None:
            continue
        if k not in known:
            raise ValueError(f"unknown option {k!r}")
        values[k] = _coerce(known[k], v)
    return GaleConfig(**values).validate()


def field_names() -> List[str]:
    return [f.name for f in fields(GaleConfig)]
