/* Host-side checks of the error paths of the real-valued-field entry points
 * (ABI v15: hbx_simulate_real / hbx_propagate_real).  Built with clang
 * -fsanitize=address against libhbx_asan.so (the library with its host code
 * ASan-instrumented) by tests/test_real_field_host.py; needs no GPU: every call
 * below returns from argument validation, before the plan is read and before
 * any HIP call. */
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
  static float values[64], target[64], field[128], inten[64];
  static double stats[3], psnr[1];

  CHECK(hbx_abi_version() == HBX_ABI_VERSION);
  CHECK(HBX_ABI_VERSION >= 15);

  /* null plan */
  CHECK(hbx_simulate_real(NULL, values, 1, field, inten, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "null plan") != NULL);
  CHECK(hbx_propagate_real(NULL, values, target, 1, inten, stats, psnr, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "null plan") != NULL);
  CHECK(hbx_simulate_real(NULL, NULL, 0, NULL, NULL, NULL) == HBX_ERR_INVALID);
  CHECK(hbx_propagate_real(NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL) == HBX_ERR_INVALID);

  /* null buffers */
  CHECK(hbx_simulate_real(plan, NULL, 1, field, inten, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "null buffer") != NULL);
  CHECK(hbx_simulate_real(plan, values, 1, NULL, inten, NULL) == HBX_ERR_INVALID);
  CHECK(hbx_propagate_real(plan, NULL, target, 1, inten, stats, psnr, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "null buffer") != NULL);
  CHECK(hbx_propagate_real(plan, values, NULL, 1, inten, stats, psnr, NULL) == HBX_ERR_INVALID);
  CHECK(hbx_propagate_real(plan, values, target, 1, inten, NULL, psnr, NULL) == HBX_ERR_INVALID);

  /* negative n_env */
  CHECK(hbx_simulate_real(plan, values, -1, field, inten, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "n_env") != NULL);
  CHECK(hbx_propagate_real(plan, values, target, -3, inten, stats, psnr, NULL) == HBX_ERR_INVALID);
  CHECK(strstr(hbx_last_error(), "n_env") != NULL);

  /* n_env == 0: nothing to do, null buffers allowed (as hbx_simulate / hbx_propagate) */
  CHECK(hbx_simulate_real(plan, NULL, 0, NULL, NULL, NULL) == HBX_OK);
  CHECK(hbx_simulate_real(plan, values, 0, field, inten, NULL) == HBX_OK);
  CHECK(hbx_propagate_real(plan, NULL, NULL, 0, NULL, NULL, NULL, NULL) == HBX_OK);
  CHECK(hbx_propagate_real(plan, values, target, 0, inten, stats, psnr, NULL) == HBX_OK);

  printf(fails ? "FAILED %d\n" : "OK\n", fails);
  return fails != 0;
}
