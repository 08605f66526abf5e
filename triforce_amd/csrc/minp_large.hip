// tf_minp_probs_large: the MINP instances of topp_large_kernel and their entry, compiled from
// csrc/topp_large.hip as a translation unit of their own so that the instances without min-p keep their instruction streams.
#define TOPP_LARGE_MINP_ENTRY
#include "topp_large.hip"
