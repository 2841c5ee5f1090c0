/* Plain-C99 consumer of include/session/fsnp_window_stream.h: the session header is valid C, libfsnp_hip.so exports its entry points
 * with C linkage, and the session's scheduling rule answers without a GPU.  Built and run by
 * tests/test_host_window_stream.py::test_header_is_plain_c_and_links_from_c. */
#include <stdio.h>

#include "session/fsnp_window_stream.h"

int main(void) {
    int64_t first[4] = {-7, -7, -7, -7}, num[4] = {-7, -7, -7, -7};
    fsnp_window_stream* ws = NULL;
    /* W = 4096, V = 1024 (S = 3072): window k is complete at 3072 k + 4096 samples */
    const int ok[4] = {fsnp_window_stream_plan(0, 4095, 4096, 1024, &first[0], &num[0]), fsnp_window_stream_plan(4095, 1, 4096, 1024, &first[1], &num[1]),
                       fsnp_window_stream_plan(4096, 6149, 4096, 1024, &first[2], &num[2]), fsnp_window_stream_plan(10000, 0, 4096, 1024, &first[3], &num[3])};
    const int bad[4] = {fsnp_window_stream_plan(0, 1, 1, 1, &first[0], &num[0]), fsnp_window_stream_plan(0, 1, 4096, 2049, &first[0], &num[0]),
                        fsnp_window_stream_plan(-1, 1, 4096, 1024, &first[0], &num[0]), fsnp_window_stream_plan(0, 1, 4096, 1024, NULL, &num[0])};
    /* a NULL handle is refused with code 1 and a message that names the call: the symbol links and answers without a device */
    const int rc = fsnp_window_stream_create(NULL, 1, 4096, 1024, 160, 32, &ws);
    printf("ok=%d,%d,%d,%d bad=%d,%d,%d,%d plan=%lld+%lld,%lld+%lld,%lld+%lld,%lld+%lld delay=%d null rc=%d msg=%s\n", ok[0], ok[1], ok[2], ok[3],
           bad[0], bad[1], bad[2], bad[3], (long long)first[0], (long long)num[0], (long long)first[1], (long long)num[1], (long long)first[2],
           (long long)num[2], (long long)first[3], (long long)num[3], fsnp_window_stream_delay(NULL), rc, fsnp_last_error());
    return (ok[0] == 0 && ok[1] == 0 && ok[2] == 0 && ok[3] == 0 && bad[0] == -1 && bad[1] == -1 && bad[2] == -1 && bad[3] == -1 && first[0] == 0 &&
            num[0] == 0 && first[1] == 0 && num[1] == 1 && first[2] == 1 && num[2] == 2 && first[3] == 2 && num[3] == 0 && rc == 1 && ws == NULL)
               ? 0 : 2;
}
