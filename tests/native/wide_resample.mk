# CPU-only program of tests/test_wide_resample_model.py (g++, no GPU, no HIP); run as `make -C tests/native -f wide_resample.mk`.
# The run geometry of a resampler plan (lsn_resample.h, header only): lanes per output, outputs and staged samples per run, under the address and
# undefined-behaviour sanitizers like _build/test_resample_cell of the Makefile next to this file.
CXX ?= g++
H = ../../ltesniffer_amd/csrc/host
all: _build/test_resample_geometry
_build/test_resample_geometry: test_resample_geometry.cc $(H)/lsn_resample.h
	mkdir -p _build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ test_resample_geometry.cc
