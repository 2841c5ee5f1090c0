/* Plain-C99 consumer of include/ext/fsnp_windowed.h: the extension header is valid C, libfsnp_hip.so exports its entry points with C
 * linkage, and the host arithmetic of the plan answers without a GPU.  Built and run by
 * tests/test_host_windowed.py::test_header_is_plain_c_and_links_from_c. */
#include <stdio.h>

#include "ext/fsnp_windowed.h"

int main(void) {
    const long long bad[4] = {(long long)fsnp_window_count(10000, 1, 1), (long long)fsnp_window_count(10000, 4096, 0),
                              (long long)fsnp_window_count(10000, 4096, 2049), (long long)fsnp_window_count(0, 4096, 1024)};
    const long long k[4] = {(long long)fsnp_window_count(10000, 4096, 1024), (long long)fsnp_window_count(4096, 4096, 1024),
                            (long long)fsnp_window_count(4097, 4096, 1024), (long long)fsnp_window_count(700, 4096, 2048)};
    /* a NULL handle is refused with code 1 and a message that names the call: the symbol links and answers without a device */
    const int rc = fsnp_enhance_wave_windowed(NULL, NULL, 0, 0, 1, NULL, 0, 0, 1, NULL, 1, 10000, 4096, 1024, 32, NULL, NULL);
    printf("bad=%lld,%lld,%lld,%lld K=%lld,%lld,%lld,%lld null rc=%d msg=%s\n", bad[0], bad[1], bad[2], bad[3], k[0], k[1], k[2], k[3], rc,
           fsnp_last_error());
    return (bad[0] == -1 && bad[1] == -1 && bad[2] == -1 && bad[3] == -1 && k[0] == 3 && k[1] == 1 && k[2] == 2 && k[3] == 1 && rc == 1) ? 0 : 2;
}
