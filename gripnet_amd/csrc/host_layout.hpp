// The pure host-side layout code of the plan builders: which edge goes into which slot of which stream.  One header per
// plan (each .hip file includes the one it uses); this umbrella includes them all for the stand-alone programs that run
// every builder - tests/host_layout_san.cpp under the sanitizers (`make -C gripnet_amd/csrc
// SAN=asan|tsan san`) and tools/probes/*_host_time.cpp.
#pragma once

#include "host_parallel.hpp"
#include "layout_util.hpp"
#include "layout_decoder.hpp"
#include "layout_decoder_bwd.hpp"
#include "layout_rgcn_pair.hpp"
#include "layout_rgcn_basis.hpp"
#include "layout_rgcn_fast.hpp"
#include "layout_blocked.hpp"
#include "layout_rel_grad.hpp"
