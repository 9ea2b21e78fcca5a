/* every public header is valid C11 on its own terms (compiled with -Wall -Wextra -pedantic, never linked) */
#include "v2v_hip.h"
#include "v2v_nernet.h"
#include "v2v_metrics.h"
#include "v2v_lpips_alex.h"
#include "v2v_alex_train.h"
