# CPU-only program of tests/test_front_source.py (g++, no GPU, no HIP); run as `make -C tests/native -f front_source.mk`.
# The ring rule and the window rule of a front-end launch's source (lsn_front_source.h, header only), under the address and undefined-behaviour sanitizers like
# _build/test_resample_geometry of wide_resample.mk next to this file.
CXX ?= g++
H = ../../ltesniffer_amd/csrc/host
all: _build/test_front_source
_build/test_front_source: test_front_source.cc $(H)/lsn_front_source.h
	mkdir -p _build
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -o $@.$$$$ test_front_source.cc && mv $@.$$$$ $@   # two pytest workers may build at once
