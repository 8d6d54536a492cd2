// What the translation units of the dev-only block library (libt2l_blocks.so: train_blocks.hip, pointnet_blocks.hip, fine_blocks.hip, fine_train_blocks.hip, text_head_blocks.hip) share: one
// thread-local error text behind t2l_blk_last_error. Defined in train_blocks.hip.
#pragma once
#include <string>

namespace t2l {

int blk_refuse(const std::string& msg);  // keeps the message, returns -1
int blk_finish(const char* who);         // hipGetLastError + a synchronise of the null stream: 0, or -2 with the message kept

}  // namespace t2l
