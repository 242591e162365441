/* Host-side checks of the error paths of the complex-field entry point
 * (hbx_simulate_complex, ABI v15 additive).  Built with clang -fsanitize=address
 * against libhbx_asan.so (the library with its host code ASan-instrumented) by
 * tests/test_complex_field_host.py; needs no GPU: every call below returns from
 * argument validation, before the plan is read and before any HIP call. */
#include <stdio.h>
#include <string.h>

#include "hbx.h"

static int fails = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      printf("FAIL line %d: %s (last error: %s)\n", __LINE__, #cond,     \
             hbx_last_error());                                          \
      fails++;                                                           \
    }                                                                    \
  } while (0)

int main(void) {
  /* a non-null plan handle for the checks that come after the null-plan check: zeroed
   * storage, which none of the calls below reads (they fail on the arguments first) */
  static long long plan_storage[1024];
  hbx_plan_t plan = (hbx_plan_t)plan_storage;
  static float values[128], field[128], real_part[64];

  CHECK(hbx_abi_version() == HBX_ABI_VERSION);
  CHECK(HBX_ABI_VERSION == 15);

  /* null plan */
  CHECK(hbx_simulate_complex(NULL, values, 1, field, real_part, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "null plan") != NULL);
  CHECK(hbx_simulate_complex(NULL, NULL, 0, NULL, NULL, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "null plan") != NULL);

  /* null values */
  CHECK(hbx_simulate_complex(plan, NULL, 1, field, real_part, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "null buffer") != NULL);

  /* both outputs null; one of the two is enough to get past the check, so those calls are
   * not made here (they would read the plan) */
  CHECK(hbx_simulate_complex(plan, values, 1, NULL, NULL, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "null buffer") != NULL);

  /* negative n_env */
  CHECK(hbx_simulate_complex(plan, values, -1, field, real_part, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "n_env") != NULL);

  /* n_env == 0: nothing to do, null buffers allowed (as hbx_simulate_real) */
  CHECK(hbx_simulate_complex(plan, NULL, 0, NULL, NULL, NULL) == HBX_OK);
  CHECK(hbx_simulate_complex(plan, values, 0, field, real_part, NULL) == HBX_OK);

  printf(fails ? "FAILED %d\n" : "OK\n", fails);
  return fails != 0;
}
