# rt355 build: the gfx950 C-ABI library, the N-API shim, the CPU oracle (test infrastructure).
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
CSRC     := compute_raytracer_amd/csrc
LIB      := compute_raytracer_amd/librt355.so
HIPFLAGS := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -fno-fast-math -Wall -Wno-unused-function $(EXTRA)
SRCS     := $(sort $(wildcard $(CSRC)/*.hip $(CSRC)/*.h)) include/rt355.h
# identity of the build: profiles (profiles/traffic.json) are evidence for the sources they were taken with
BUILD_ID := $(shell cat $(SRCS) | sha256sum | cut -c1-16)
OBJS     := $(CSRC)/rt_api.o $(CSRC)/rt_kernels.o $(CSRC)/rt_bvh.o $(CSRC)/rt_triangles.o $(CSRC)/rt_assemble.o $(CSRC)/rt_comm.o $(CSRC)/rt_query.o $(CSRC)/rt_shade.o $(CSRC)/rt_sample.o $(CSRC)/rt_gbuffer.o $(CSRC)/rt_ao.o $(CSRC)/rt_refit.o $(CSRC)/rt_build.o $(CSRC)/rt_tlas.o $(CSRC)/rt_closest.o $(CSRC)/rt_deform.o

all: lib oracle node

lib: $(LIB)

# the ray-trace kernels: no FMA contraction, no SLP (packed-math) vectorisation -- see the
# header of rt_kernels.hip
$(CSRC)/rt_kernels.o: $(CSRC)/rt_kernels.hip $(CSRC)/rt_filter.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

$(CSRC)/rt_bvh.o: $(CSRC)/rt_bvh.hip $(CSRC)/rt_filter.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

$(CSRC)/rt_triangles.o: $(CSRC)/rt_triangles.hip $(CSRC)/rt_tri_device.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h $(CSRC)/rt_tri_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# ray queries: the triangle kernel's traversal and the literal sphere test, the same flags (exactness rests on them)
$(CSRC)/rt_query.o: $(CSRC)/rt_query.hip $(CSRC)/rt_query_device.h $(CSRC)/rt_query_form.h $(CSRC)/rt_tri_device.h $(CSRC)/rt_filter.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h $(CSRC)/rt_tri_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# shaded ray queries: the frame kernels' bounce loop over caller rays, rt_query.o's flags exactly (exactness rests on them)
$(CSRC)/rt_shade.o: $(CSRC)/rt_shade.hip $(CSRC)/rt_shade_device.h $(CSRC)/rt_query_device.h $(CSRC)/rt_query_form.h $(CSRC)/rt_tri_device.h $(CSRC)/rt_filter.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h $(CSRC)/rt_tri_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# supersampled frames: rt_shade.o's bounce loops from the camera, resolved on the chip; rt_shade.o's flags exactly
$(CSRC)/rt_sample.o: $(CSRC)/rt_sample.hip $(CSRC)/rt_shade_device.h $(CSRC)/rt_query_device.h $(CSRC)/rt_query_form.h $(CSRC)/rt_tri_device.h $(CSRC)/rt_filter.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h $(CSRC)/rt_tri_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# geometry frames: rt_query.o's walks from the camera, stored as planes; rt_query.o's flags exactly (exactness rests on them)
$(CSRC)/rt_gbuffer.o: $(CSRC)/rt_gbuffer.hip $(CSRC)/rt_shade_device.h $(CSRC)/rt_query_device.h $(CSRC)/rt_query_form.h $(CSRC)/rt_tri_device.h $(CSRC)/rt_filter.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h $(CSRC)/rt_tri_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# ambient-occlusion frames: rt_gbuffer.o's primary walk, then rt_query.o's occlusion walks from the hit; the same flags exactly
$(CSRC)/rt_ao.o: $(CSRC)/rt_ao.hip $(CSRC)/rt_shade_device.h $(CSRC)/rt_query_device.h $(CSRC)/rt_query_form.h $(CSRC)/rt_tri_device.h $(CSRC)/rt_filter.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h $(CSRC)/rt_tri_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# the BLAS refit: float32 min / max only, nothing to contract
$(CSRC)/rt_refit.o: $(CSRC)/rt_refit.hip $(CSRC)/rt_refit.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -c $< -o $@

# the device BLAS build: float64 planes, areas and costs that must equal the host builder's bit for bit -- no FMA contraction, no
# SLP vectorisation (exactness rests on them); rt_blas_build.h holds the arithmetic and is shared with the host model
$(CSRC)/rt_build.o: $(CSRC)/rt_build.hip $(CSRC)/rt_build.h $(CSRC)/rt_blas_build.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# the device top-level build's front end: float64 cofactors and corner transforms that must equal the host model's bit for bit;
# rt_build.o's flags exactly.  rt_tlas_build.h holds the arithmetic and is shared with the host model
$(CSRC)/rt_tlas.o: $(CSRC)/rt_tlas.hip $(CSRC)/rt_tlas_build.h $(CSRC)/rt_build.h $(CSRC)/rt_blas_build.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# closest-point queries: float64 leaves that must equal the host model's bit for bit; rt_query.o's flags exactly.  rt_closest.h
# holds the arithmetic and the walk and is shared with the host model
$(CSRC)/rt_closest.o: $(CSRC)/rt_closest.hip $(CSRC)/rt_closest.h $(CSRC)/rt_tlas_build.h $(CSRC)/rt_blas_build.h $(CSRC)/rt_query_device.h $(CSRC)/rt_query_form.h $(CSRC)/rt_tri_device.h $(CSRC)/rt_device.h $(CSRC)/rt_types.h $(CSRC)/rt_tri_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

# device mesh deformation: float32 flat normals that must equal the host model's bit for bit; the exact kernels' flags.
# rt_deform.h holds the arithmetic and is shared with the host model
$(CSRC)/rt_deform.o: $(CSRC)/rt_deform.hip $(CSRC)/rt_deform.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -fno-slp-vectorize -c $< -o $@

$(CSRC)/rt_assemble.o: $(CSRC)/rt_assemble.hip $(CSRC)/rt_types.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(CSRC)/rt_api.o: $(SRCS)
	$(HIPCC) $(HIPFLAGS) -ffp-contract=off -DRT355_BUILD_ID='"$(BUILD_ID)"' -c $(CSRC)/rt_api.hip -o $@

# the RCCL entry points (rt_comm_init / rt_render_gather / rt_group_*)
$(CSRC)/rt_comm.o: $(CSRC)/rt_comm.hip $(CSRC)/rt_ctx.h $(CSRC)/rt_own.h $(CSRC)/rt_flow_build.h $(CSRC)/rt_types.h $(CSRC)/rt_tri_types.h $(CSRC)/rt_wait_poll.h $(CSRC)/rt_exchange_plan.h include/rt355.h
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) -o $@ $(OBJS) -L/opt/rocm/lib -lrccl

oracle:
	$(MAKE) -s -C oracle

node:
	@if [ -f node/Makefile ]; then $(MAKE) -s -C node; fi

clean:
	rm -f $(OBJS) $(LIB)
	$(MAKE) -s -C oracle clean
	@if [ -f node/Makefile ]; then $(MAKE) -s -C node clean; fi

.PHONY: all lib oracle node clean
