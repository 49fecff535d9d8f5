# The build of a companion library, included by ../recon, ../map, ../typed, ../requant and ../views (each Makefile sets NAME and FUSED;
# ALSO, where set, names further files its units include -- dependencies only, no flag and no source changes with it):
# rustyhgi_amd/libhgi_$(NAME).so for gfx950 (MI355X) from the directory's entry unit and kernel unit.  Same flags as ../csrc/Makefile; the kernels
# include the codec's tile procedure from ../csrc -- FUSED is the direction's unit, hgi_fused_enc.hip or hgi_fused_dec.hip --
# without modifying it, and nothing of libhgi_hip.so is linked.  hipcc cross-compiles without a GPU.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
# -fvisibility=hidden + the version script: the shared object exports the hgi_$(NAME)_* entry points of include/hgi_$(NAME).h only
CXXFLAGS ?= -O3 -std=c++17 -fPIC -fvisibility=hidden -fvisibility-inlines-hidden -Wall -Wextra -Wno-unused-parameter
# experiment builds: make VARIANT=_x EXTRA='-D...' -> ../libhgi_$(NAME)_x.so
VARIANT ?=
EXTRA ?=
ALSO ?=
OUT := ../libhgi_$(NAME)$(VARIANT).so
OBJ := _obj$(VARIANT)
CSRC := ../csrc
COMPANION := ../companion

all: $(OUT)

$(OBJ)/%.o: %.hip hgi_$(NAME)_plan.h hgi_$(NAME)_kernels.h $(COMPANION)/hgi_sides.h $(COMPANION)/hgi_entry.h $(COMPANION)/hgi_tile.h $(CSRC)/hgi_kernels.h $(CSRC)/hgi_dev.h $(CSRC)/hgi_fused_impl.h $(CSRC)/$(FUSED) $(CSRC)/hgi_fastdiv.h $(CSRC)/hgi_tilewalk.h $(CSRC)/hgi_pitched.h $(CSRC)/hgi_fused_pitched.h $(CSRC)/hgi_knobs.h $(CSRC)/hgi_launch_policy.h $(CSRC)/hgi_launch.h $(CSRC)/hgi_dec_chain.h ../../include/hgi.h ../../include/hgi_$(NAME).h $(ALSO)
	@mkdir -p $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) $(EXTRA) -c $< -o $@

$(OUT): $(OBJ)/hgi_$(NAME).o $(patsubst %.hip,$(OBJ)/%.o,$(wildcard hgi_fused_*.hip)) hgi_$(NAME).map
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,--version-script=hgi_$(NAME).map -o $@ $(filter %.o,$^)

clean:
	rm -rf $(OBJ) $(OUT)
.PHONY: all clean
