// ngp_field_input_grad_pm: inputgrad.hip's field_input_grad kernel on the training
// step's pair-major saved encoding (see the note at the top of inputgrad.hip).
#define NGP_ENC_PAIR_MAJOR 1
#include "inputgrad.hip"
