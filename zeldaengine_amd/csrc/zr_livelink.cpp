// zr_livelink.cpp — the TCP livelink server.
//
// Replaces the socket listener thread (ZE:1617-1710, WinSock only in the reference: the #else branch is "@TODO: Implement for macOS and
// Linux").  The wire contract is kept: IPv4 TCP, one recv of <= 65720 bytes per connection holding the whole JSON, no reply bytes,
// shutdown(SHUT_WR).  The reference parses on the socket thread straight into the live World (a data race, ZE:1687 vs 4296); here the
// listener parses into a private ZrWorld (zr_world_doc.cpp) and zr_livelink_poll swaps it in on the render thread, which is DrawFrame's
// bReloadScene pickup (ZE:1943-1951).
#include "zr_ctx.h"

#include <arpa/inet.h>
#include <netinet/in.h>
#include <poll.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>

// One connection: wait (in 100 ms slices, so that zr_livelink_stop is never held up by a silent client) for the first
// segment, then ONE recv (ZE:1683).  A client that sends nothing within XK_LIVELINK_IDLE_MS is dropped.
#define XK_LIVELINK_IDLE_MS 2000
static void livelink_thread(zr_ctx* c)
{
    std::vector<char> buf;
    try { buf.resize(XK_LIVELINK_RECV_MAX); } catch (...) { fprintf(stderr, "[Socket] out of memory: not serving\n"); return; }
    while (c->ll_run.load()) {
        struct pollfd pfd = { c->ll_listen_fd, POLLIN, 0 };
        const int pr = poll(&pfd, 1, 100);
        if (pr <= 0 || !(pfd.revents & POLLIN)) continue;
        const int cs = accept(c->ll_listen_fd, nullptr, nullptr);
        if (cs < 0) { fprintf(stderr, "[Socket] accept failed\n"); continue; }      // keep listening, ZE:1676-1679
        ssize_t n = -2;                                                                // -2: timed out / stopping
        try {       // (nothing may leave this thread: an exception here would end the host's process)
            for (int waited = 0; waited < XK_LIVELINK_IDLE_MS && c->ll_run.load(); waited += 100) {
                struct pollfd cfd = { cs, POLLIN, 0 };
                const int cr = poll(&cfd, 1, 100);
                if (cr < 0) { n = -1; break; }
                if (cr > 0) { n = recv(cs, buf.data(), buf.size(), 0); break; }            // ONE recv per connection, ZE:1683
            }
            if (n > 0) {
                ZrWorld w; std::string err;
                if (zr_world_parse(buf.data(), (size_t)n, w, err)) {
                    std::lock_guard<std::mutex> g(c->ll_mutex);
                    c->ll_world = std::move(w); c->ll_pending = true;                    // World.bReloadScene = true, ZE:4290
                } else {
                    // the engine throws on the socket thread here (ZE:1071-1073) and dies; the library logs and keeps serving
                    fprintf(stderr, "%s\n", err.c_str());
                }
            } else if (n == 0) fprintf(stdout, "[Socket] Connection closing...\n");
            else if (n == -2) fprintf(stderr, "[Socket] client sent nothing: dropped\n");
            else fprintf(stderr, "[Socket] recv failed\n");
        } catch (...) { fprintf(stderr, "[Socket] payload dropped: out of memory or an unexpected exception\n"); }
        shutdown(cs, SHUT_WR);                                                        // no payload is ever sent back, ZE:1699
        close(cs);
    }
}

// The engine binds the wildcard address (AI_PASSIVE, ZE:1630-1636); the payload is unauthenticated, so the library listens on
// loopback unless the host asks for the engine's behaviour with zr_livelink_bind_any(ctx, 1) before zr_livelink_serve.
extern "C" int zr_livelink_bind_any(zr_ctx* c, int any)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->ll_bind_any = any != 0;
        return ZR_OK;
    });
}

// zr_livelink_poll applies a payload as a difference against the live world (zr_world_update_json) instead of loading it
extern "C" int zr_livelink_set_incremental(zr_ctx* c, int on)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        c->ll_incremental = on != 0;
        return ZR_OK;
    });
}

extern "C" int zr_livelink_serve(zr_ctx* c, uint16_t port)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (c->ll_run.load()) return zr_fail(c, ZR_ERR_STATE, "livelink already serving");
        const int fd = socket(AF_INET, SOCK_STREAM, IPPROTO_TCP);
        if (fd < 0) return zr_fail(c, ZR_ERR_IO, "[Socket] socket failed");
        int one = 1; setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
        struct sockaddr_in a; memset(&a, 0, sizeof a);
        a.sin_family = AF_INET; a.sin_addr.s_addr = htonl(c->ll_bind_any ? INADDR_ANY : INADDR_LOOPBACK); a.sin_port = htons(port);
        if (bind(fd, (struct sockaddr*)&a, sizeof a) < 0) { close(fd); return zr_fail(c, ZR_ERR_IO, "[Socket] bind failed"); }
        if (listen(fd, SOMAXCONN) < 0) { close(fd); return zr_fail(c, ZR_ERR_IO, "[Socket] listen failed"); }
        socklen_t al = sizeof a;
        if (getsockname(fd, (struct sockaddr*)&a, &al) == 0) c->ll_port = ntohs(a.sin_port);
        c->ll_listen_fd = fd; c->ll_run.store(true);
        c->ll_thread = std::thread(livelink_thread, c);
        return ZR_OK;
    });
}

extern "C" int zr_livelink_port(zr_ctx* c, uint16_t* port) { if (!c || !port) return ZR_ERR_ARG; return zr_guard(c, [&]() -> int { *port = c->ll_port; return ZR_OK; }); }

extern "C" int zr_livelink_poll(zr_ctx* c, int* reloaded)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (reloaded) *reloaded = 0;
        ZrWorld w; bool have = false;
        { std::lock_guard<std::mutex> g(c->ll_mutex); if (c->ll_pending) { w = std::move(c->ll_world); c->ll_pending = false; have = true; } }
        if (!have) return ZR_OK;
        if (c->ll_incremental) {        // zr_livelink_set_incremental: only what differs from the live scene
            zr_world_delta D;
            const int rc = zr_update_world_guarded(c, w, D);
            if (rc == ZR_OK && reloaded) *reloaded = 1;
            return rc;
        }
        (void)hipSetDevice(c->device);
        if (zr_sync_all(c) != hipSuccess) return zr_fail(c, ZR_ERR_DEVICE, "livelink: device synchronisation failed");   // "wait all fences" on both lanes before CreateEngineScene, ZE:1943-1951
        int rc = zr_apply_world_guarded(c, w);
        if (rc == ZR_OK && reloaded) *reloaded = 1;
        return rc;
    });
}

extern "C" int zr_livelink_stop(zr_ctx* c)
{
    if (!c) return ZR_ERR_ARG;
    return zr_guard(c, [&]() -> int {
        if (!c->ll_run.load()) return ZR_OK;
        c->ll_run.store(false);
        if (c->ll_thread.joinable()) c->ll_thread.join();
        if (c->ll_listen_fd >= 0) { close(c->ll_listen_fd); c->ll_listen_fd = -1; }
        return ZR_OK;
    });
}
