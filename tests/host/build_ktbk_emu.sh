#!/bin/bash
# Builds the host-emulated stage harness of the Bloom keys (tests/kernels/stage_harness_bloom_keys.hip: the engine
# plus the entry point that launches P1b for keys of two to four words alone), compiled by g++ against tests/host/hip_emu
# like build_emu.sh's engine.
# TEST INFRASTRUCTURE: loaded only by tests/test_bloom_keys_part_emu.py (JFKTBK_LIB); never measured, never shipped.
set -e
cd "$(dirname "$0")/../.."
mkdir -p tests/host/_build
# up to date?
if [ -f tests/host/_build/libjfgpu_ktbk_emu.so ] && \
   [ -z "$(find jellyfish_amd/csrc include tests/host/hip_emu tests/host/build_ktbk_emu.sh tests/kernels/stage_harness_bloom_keys.hip -type f -newer tests/host/_build/libjfgpu_ktbk_emu.so -print -quit)" ]; then
  exit 0
fi
g++ -std=c++17 -O2 -g -x c++ -DJFGPU_EMU -Itests/host/hip_emu -fPIC -shared -pthread \
    -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result -Wno-unknown-pragmas -Wno-sign-compare -Wno-unused-but-set-variable -Wno-unused-variable \
    -o tests/host/_build/libjfgpu_ktbk_emu.so tests/kernels/stage_harness_bloom_keys.hip
