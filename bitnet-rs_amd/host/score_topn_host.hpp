// score_topn_host.hpp -- the C export of Decoder::score_topn (decoder.hpp), defined in decoder.cpp's extern "C" tail beside bitnet_host_score.
// d: a decoder from bitnet_host_create / _create_shared.
#pragma once

extern "C" {
// records_out: n bitnet_hip_logprob_record; nll_out: n - 1 floats or NULL
int bitnet_host_score_topn(void *d, int n, int digits, int top_n, void *records_out, float *nll_out, float *elapsed_ms);
}
