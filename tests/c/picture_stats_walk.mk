# The host code of the picture statistics under ASan + UBSan (tests/test_picture_stats_host_sanitized.py): picture_stats_walk.cpp, a plain
# C++ program with its own main, compiled host-only with the sanitizer and linked with the OBJECTS of the device-free
# sanitizer build of the library (make -C schroedinger_amd/csrc dry_asan leaves them in dry_asan/) -- one image, the
# sanitizer's runtime linked into the program itself, nothing preloaded.  Needs no device; -fno-gpu-sanitize says outright
# that the sanitizer is for the host code alone.
#   make -f picture_stats_walk.mk picture_stats_walk_asan
ROOT = ../..
CSRC = $(ROOT)/schroedinger_amd/csrc
LIBDIR = $(ROOT)/schroedinger_amd
HIPCC ?= /opt/rocm/bin/hipcc
WALKFLAGS = -O1 -g -fno-omit-frame-pointer -std=c++17 -Wall -I$(ROOT)/include

picture_stats_walk_asan: _build/picture_stats_walk_asan

# (the library's own Makefile decides whether its objects are up to date)
$(LIBDIR)/libschro_hip_dry_asan.so: FORCE
	$(MAKE) -C $(CSRC) dry_asan
FORCE:

_build/picture_stats_walk_asan: picture_stats_walk.cpp $(ROOT)/include/schro_hip.h $(LIBDIR)/libschro_hip_dry_asan.so
	mkdir -p _build
	$(HIPCC) --offload-host-only -x c++ $(WALKFLAGS) -fsanitize=address,undefined -fno-gpu-sanitize -fno-sanitize=vptr,function -c picture_stats_walk.cpp -o _build/picture_stats_walk_asan.o
	$(HIPCC) -fsanitize=address,undefined -fno-gpu-sanitize _build/picture_stats_walk_asan.o $(CSRC)/dry_asan/*.o -lpthread -o $@

.PHONY: picture_stats_walk_asan FORCE
