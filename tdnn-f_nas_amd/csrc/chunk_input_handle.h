// chunk_input_handle.h -- the handle of the chunk minibatch inputs (include/tdnnf_hip.h, "CHUNK INPUTS"), for the two files that stage a
// minibatch's table through its ring: chunk_input.hip (the float gather) and feature_store.hip (the gather out of a feature store).
#pragma once
#include "assign_stage.h"

struct tdnnf_chunk_input {
  int max_sequences;
  tdnnf::AssignStage stage;  // the device table is the whole of its allocation
  int allocs_at_create;
  long long gathers;
  int last_form;  // of the last gather: 4 the 16-byte form, 1 the scalar form, 0 before the first
};
