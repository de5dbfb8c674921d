# gale native build: hand-written gfx950 HIP kernels + C++ host runtime -> gale/_C.so
# (in-tree, so the built library travels with the repo snapshot to the GPU box).
ROCM      ?= /opt/rocm
HIPCC     ?= $(ROCM)/bin/hipcc
CXX       ?= g++
ARCH      ?= gfx950
PYTHON    ?= python3
PY_INC    := $(shell $(PYTHON) -c "import sysconfig;print(sysconfig.get_paths()['include'])")
PYBIND_INC:= $(shell $(PYTHON) -c "import pybind11;print(pybind11.get_include())")
OBJ       := build/obj

HIP_FLAGS := --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Icsrc/include -Icsrc/kernels \
             -Wno-unused-result
CXX_FLAGS := -O3 -fPIC -std=c++17 -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Icsrc/include \
             -I$(PY_INC) -I$(PYBIND_INC) -mavx2 -mfma -msse4.2 -mpclmul -mbmi2 -pthread \
             -fvisibility=hidden -Wall -Wno-unused-function -Wno-unused-result

HIP_SRC   := $(wildcard csrc/kernels/*.hip)
CXX_SRC   := $(wildcard csrc/runtime/*.cpp) $(wildcard csrc/codec/*.cpp) \
             $(wildcard csrc/kafka/*.cpp) $(wildcard csrc/comm/*.cpp) $(wildcard csrc/bindings/*.cpp)
HIP_OBJ   := $(patsubst csrc/%.hip,$(OBJ)/%.o,$(HIP_SRC))
CXX_OBJ   := $(patsubst csrc/%.cpp,$(OBJ)/%.o,$(CXX_SRC))
HDRS      := $(wildcard csrc/include/gale/*.h) $(wildcard csrc/kernels/*.cuh) \
             $(wildcard csrc/kernels/*.h) \
             $(wildcard csrc/runtime/*.h) $(wildcard csrc/codec/*.h) $(wildcard csrc/kafka/*.h) \
             $(wildcard csrc/comm/*.h) $(wildcard csrc/bindings/*.h)

all: gale/_C.so

$(OBJ)/%.o: csrc/%.hip $(HDRS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIP_FLAGS) -c $< -o $@

$(OBJ)/%.o: csrc/%.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(CXX) $(CXX_FLAGS) -c $< -o $@

gale/_C.so: $(HIP_OBJ) $(CXX_OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ -L$(ROCM)/lib -lamdhip64 -lrccl -lrocprofiler-sdk-roctx -lz -ldl -pthread \
	    -Wl,-rpath,$(ROCM)/lib

clean:
	rm -rf build gale/_C.so

.PHONY: all clean

# ---- host-pipeline sanitizer builds: engine + Kafka client/broker + codec with
# CPU stub replicas under ThreadSanitizer / AddressSanitizer. Host code only (no GPU code is
# linked; GPU sanitizers are not available on this pool).
SAN_SRC   := csrc/tests/engine_stress.cpp csrc/runtime/engine.cpp csrc/runtime/replica.cpp \
             csrc/runtime/resize_plan.cpp csrc/runtime/pinned_pool.cpp csrc/runtime/trace.cpp \
             csrc/codec/json_codec.cpp csrc/codec/text_pack.cpp csrc/codec/java8_float.cpp \
             csrc/codec/resize.cpp \
             $(wildcard csrc/kafka/*.cpp)
SAN_FLAGS := -O1 -g -fno-omit-frame-pointer -std=c++17 -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include \
             -Icsrc/include -mavx2 -mfma -msse4.2 -mpclmul -mbmi2 -pthread
SAN_LIBS  := -L$(ROCM)/lib -lamdhip64 -lrocprofiler-sdk-roctx -lz -ldl -Wl,-rpath,$(ROCM)/lib
# LLVM's sanitizer runtimes (ROCm's clang): gcc-11's libtsan does not intercept
# pthread_cond_clockwait, which libstdc++'s condition_variable uses, and reports false races
SAN_CXX   ?= $(ROCM)/lib/llvm/bin/clang++

build/tsan/engine_stress: $(SAN_SRC) $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) $(SAN_FLAGS) -fsanitize=thread $(SAN_SRC) -o $@ $(SAN_LIBS)

build/asan/engine_stress: $(SAN_SRC) $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined $(SAN_SRC) -o $@ $(SAN_LIBS)

# the base64 record scanner / host decoder / splitter on mutated and truncated records
# (csrc/tests/b64_scan_check.cpp): codec only, no engine
build/asan/b64_scan_check: csrc/tests/b64_scan_check.cpp csrc/codec/json_codec.cpp \
                           csrc/codec/java8_float.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma -msse4.2 \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/b64_scan_check.cpp csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp -o $@

# the YUV 4:2:0 host codec (csrc/tests/yuv_check.cpp): the conversion twin, the frame-record
# decoder and the byte-count forms of the scan / offsets / splitter on mutated and truncated
# records; codec only, no engine, no HIP call
build/asan/yuv_check: csrc/tests/yuv_check.cpp csrc/codec/json_codec.cpp \
                      csrc/codec/java8_float.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma -msse4.2 \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/yuv_check.cpp csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp -o $@

# the packed-pixel host codec (csrc/tests/pixfmt_check.cpp): the unpack twin, the record decoder
# and the byte-count forms of the scan / offsets / splitter on mutated and truncated records;
# codec only, no engine, no HIP call
build/asan/pixfmt_check: csrc/tests/pixfmt_check.cpp csrc/codec/json_codec.cpp \
                         csrc/codec/java8_float.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma -msse4.2 \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/pixfmt_check.cpp csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp -o $@

# PixelSource (csrc/tests/pixel_source_check.cpp): the names, the bytes of a string, the refusals,
# the ingest's dimensions and the host dispatch against the three decoders on mutated and
# truncated records, for all seven pixel formats; codec only, no engine, no HIP call
build/asan/pixel_source_check: csrc/tests/pixel_source_check.cpp csrc/codec/json_codec.cpp \
                               csrc/codec/java8_float.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma -msse4.2 \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/pixel_source_check.cpp csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp -o $@

# typed tensor records (csrc/tests/elemtype_check.cpp): the element codec on every 16-bit pattern
# and on f32 patterns, PixelSource's fourth arm (names, bytes, refusals, ingest dimensions) and the
# typed record decoder on planted, mutated and truncated records; codec only, no engine, no HIP call
build/asan/elemtype_check: csrc/tests/elemtype_check.cpp csrc/codec/json_codec.cpp \
                           csrc/codec/java8_float.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma -msse4.2 \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/elemtype_check.cpp csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp -o $@

# the b64 ingest's host plan behind the scanner, on mutated records and mutated scan results
# (csrc/tests/b64_plan_check.cpp): codec + plan, no engine, no HIP call
build/asan/b64_plan_check: csrc/tests/b64_plan_check.cpp csrc/runtime/ingest_plan.cpp \
                           csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma -msse4.2 \
	    -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Icsrc/include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/b64_plan_check.cpp csrc/runtime/ingest_plan.cpp \
	    csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp -o $@

# the JSON ingest's host plan (layout + fill) behind the envelope scanner, on mutated records and
# mutated scan results (csrc/tests/json_plan_check.cpp): codec + plan, no engine, no HIP call
build/asan/json_plan_check: csrc/tests/json_plan_check.cpp csrc/runtime/ingest_plan.cpp \
                            csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma -msse4.2 \
	    -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Icsrc/include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/json_plan_check.cpp csrc/runtime/ingest_plan.cpp \
	    csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp -o $@

# the GPU replica's host batch plan (layout + fill) on random and mutated batches
# (csrc/tests/batch_plan_check.cpp): the plan alone, no codec, no engine, no HIP call
build/asan/batch_plan_check: csrc/tests/batch_plan_check.cpp csrc/runtime/batch_plan.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 \
	    -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Icsrc/include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/batch_plan_check.cpp csrc/runtime/batch_plan.cpp -o $@

# the forward plan's validation on randomly corrupted plans of every op kind
# (csrc/tests/forward_plan_check.cpp): the plan and the conv route, no executor, no HIP call
build/asan/forward_plan_check: csrc/tests/forward_plan_check.cpp csrc/runtime/forward_plan.cpp \
                               csrc/runtime/conv_route.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 \
	    -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Icsrc/include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/forward_plan_check.cpp csrc/runtime/forward_plan.cpp \
	    csrc/runtime/conv_route.cpp -o $@

# the conv route on random and extreme descs (csrc/tests/conv_route_check.cpp): every count a
# launcher passes as a 32-bit value recomputed in 64 bits; the route alone, no HIP header or call
build/asan/conv_route_check: csrc/tests/conv_route_check.cpp csrc/runtime/conv_route.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -Icsrc/include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/conv_route_check.cpp csrc/runtime/conv_route.cpp -o $@

# the two top-k encoders (host selection by the score order rule, slot concatenation) over
# generated rows (csrc/tests/topk_encode_check.cpp): codec only, no engine
build/asan/topk_encode_check: csrc/tests/topk_encode_check.cpp csrc/codec/json_codec.cpp \
                              csrc/codec/java8_float.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma -msse4.2 \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/topk_encode_check.cpp csrc/codec/json_codec.cpp csrc/codec/java8_float.cpp -o $@

# the input resize's table builder and host twin (csrc/tests/resize_check.cpp): every
# (source, resize, model) size of 1..24 per axis and the 4096 extremes; codec only, no HIP call
build/asan/resize_check: csrc/tests/resize_check.cpp csrc/codec/resize.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/resize_check.cpp csrc/codec/resize.cpp -o $@

# the antialiased resize's table builder and host twin (csrc/tests/resize_aa_check.cpp): every
# (source, resize, model) size of 1..24 per axis within the 8x limit, the 4096 extremes, refusal
# of every triple over the limit; codec only, no HIP call
build/asan/resize_aa_check: csrc/tests/resize_aa_check.cpp csrc/codec/resize.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/resize_aa_check.cpp csrc/codec/resize.cpp -o $@

# the input resize's host plan (csrc/tests/resize_plan_check.cpp): the device image of the tables
# (layout, padding, payloads), the bound kernel plans and the host dispatch, both forms, every
# size of 1..12 per axis and the 4096 extremes; plan + codec, no engine, no HIP call
build/asan/resize_plan_check: csrc/tests/resize_plan_check.cpp csrc/runtime/resize_plan.cpp \
                              csrc/codec/resize.cpp $(HDRS)
	@mkdir -p $(dir $@)
	$(SAN_CXX) -O1 -g -fno-omit-frame-pointer -std=c++17 -mavx2 -mfma \
	    -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -Icsrc/include \
	    -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    csrc/tests/resize_plan_check.cpp csrc/runtime/resize_plan.cpp csrc/codec/resize.cpp -o $@

tsan: build/tsan/engine_stress
	TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1" ./build/tsan/engine_stress 1500

asan: build/asan/engine_stress
	ASAN_OPTIONS="detect_leaks=1" ./build/asan/engine_stress 2000

.PHONY: tsan asan

# host codec micro-benchmark (CRC32C + envelope scan GB/s per core)
build/host_bench: csrc/tests/host_bench.cpp csrc/codec/json_codec.cpp csrc/kafka/wire.cpp $(HDRS)
	@mkdir -p build
	$(CXX) -O3 -std=c++17 -mavx2 -mfma -msse4.2 -mpclmul -mbmi2 -Icsrc/include \
	    csrc/tests/host_bench.cpp csrc/codec/json_codec.cpp csrc/kafka/wire.cpp -o $@

# DRAM antagonist for the host-projection test (tools/dram_antagonist.cpp); outside build/ so it
# travels to the GPU box (build/ is gpurun-ignored)
tools/bin/dram_antagonist: tools/dram_antagonist.cpp
	@mkdir -p tools/bin
	$(CXX) -O2 -std=c++17 -mavx2 -pthread $< -o $@

antagonist: tools/bin/dram_antagonist
.PHONY: antagonist
