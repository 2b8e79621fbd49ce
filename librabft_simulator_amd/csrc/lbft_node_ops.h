// lbft_node_ops.h -- the node-level interface (include/lbft.h lbft_node_*, lbft_node_calls): one lane applies one trait call to one
// node.  The kernels lbft_k_node_op / lbft_k_node_ops (lbft_hip.hip) run it on the device; oracle/host_model.cpp compiles the same
// body for the host so that the CPU-only tests (tests/test_node_level_fuzz.py) exercise exactly the code the product library runs.
// Included after lbft_core.h under `using namespace lbft`.
//   out[0..15]: the call's result words -- OP_UPDATE: next scheduled update, should_send (two words: authors 0-63, 64-127),
//   broadcast, query_all; OP_CREATE_* / OP_HANDLE_REQUEST: the snapshot slot or -1 when the pool is full; OP_HANDLE_NOTIFICATION:
//   should_sync; OP_VIEW: the lbft_node_view fields in declaration order.
#ifndef LBFT_NODE_OPS_H
#define LBFT_NODE_OPS_H

#if defined(__HIPCC__)
#define LBFT_NODE_OP __device__ __forceinline__
#else  // the host build of the kernel logic (oracle/host_model.cpp)
#define LBFT_NODE_OP inline
#define __popc(x) __builtin_popcount(x)
#endif

enum NodeOp : u32 { OP_UPDATE = 0, OP_CREATE_NOTIFICATION, OP_HANDLE_NOTIFICATION, OP_RELEASE_NOTIFICATION, OP_VIEW,
                    OP_CREATE_REQUEST, OP_HANDLE_REQUEST, OP_HANDLE_RESPONSE };
LBFT_NODE_OP void node_op_body(const Params& p, u32* __restrict__ state, u32 op, u32 inst, u32 node, u32 arg0, u32 arg1, i64 node_time,
                               unsigned long long* __restrict__ out) {
  Sim s(p, state, inst);
  s.load_scalars();
  if (op == OP_UPDATE) {
    s.begin_node(node);
    Actions a = s.update_node(node, node_time);
    s.end_node(node);
    out[0] = (unsigned long long)a.next;
    out[1] = out[2] = 0;
    if (a.send_to >= 0) out[1 + (a.send_to >> 6)] = 1ULL << (a.send_to & 63);
    out[3] = a.broadcast ? 1 : 0;
    out[4] = a.query_all ? 1 : 0;
  } else if (op == OP_CREATE_NOTIFICATION) {
    s.begin_node(node);
    i32 slot = s.snap_alloc();
    if (slot >= 0) { s.write_snapshot(node, (u32)slot); s.snap_set_refs((u32)slot, 1, s.nf(node, NF_EPOCH)); }
    out[0] = (unsigned long long)(long long)slot;
  } else if (op == OP_HANDLE_NOTIFICATION) {
    s.begin_node(node);
    auto sn = s.load_snapshot(arg1);
    bool sync = s.handle_notification(node, arg0, arg1, sn);
    s.end_node(node);
    out[0] = sync ? 1 : 0;
  } else if (op == OP_RELEASE_NOTIFICATION) {
    s.snap_release(arg1);
  } else if (op == OP_CREATE_REQUEST) {  // DataSyncNode::create_request (data_sync.rs:66-71,179-181): epoch + the chains' heads
    s.begin_node(node);
    i32 slot = s.make_request_slot(s.nf(node, NF_EPOCH), s.nf(node, NF_HCC_BLK) | (s.nf(node, NF_HQC_BLK) << 16));
    if (slot >= 0) s.snap_set_refs((u32)slot, 1, s.nf(node, NF_EPOCH));
    out[0] = (unsigned long long)(long long)slot;
  } else if (op == OP_HANDLE_REQUEST) {  // DataSyncNode::handle_request on `node` (data_sync.rs:183-207): its store now + the request
    s.begin_node(node);
    u32 qb = s.sfw(arg1, 0);
    u32 req_epoch = s.ld(qb + S_EPOCH), req_certs = s.ld(qb + S_CERTS);
    if (s.refpack()) req_epoch &= 0xffffu;  // (large networks: the slot's reference count rides in the upper half of this word)
    i32 slot = s.snap_alloc();
    if (slot >= 0) {
      u32 rb = s.sfw((u32)slot, 0);
      s.write_store_snapshot(node, rb);
      s.st(s.sqw(rb, 0), req_epoch); s.st(s.sqw(rb, 1), req_certs);
      s.snap_set_refs((u32)slot, 1, s.nf(node, NF_EPOCH));
    }
    out[0] = (unsigned long long)(long long)slot;
  } else if (op == OP_HANDLE_RESPONSE) {  // DataSyncNode::handle_response(response from peer arg0, clock) (data_sync.rs:209-240)
    s.begin_node(node);
    s.handle_response(node, arg0, arg1, node_time);
    s.end_node(node);
  } else {  // OP_VIEW
    s.begin_node(node);
    out[0] = s.nf(node, NF_EPOCH); out[1] = s.nf(node, NF_CUR_ROUND); out[2] = s.nf(node, NF_HQC_ROUND);
    out[3] = s.nf(node, NF_HTC_ROUND); out[4] = s.nf(node, NF_HC_ROUND); out[5] = s.nf(node, NF_PM_ROUND);
    out[6] = s.nf(node, NF_LVR); out[7] = s.nf(node, NF_LOCKED); out[8] = s.nf(node, NF_NCOMMITS);
    u32 leader = s.nf(node, NF_PM_LEADER);
    out[9] = leader == LBFT_NO_LEADER ? 0xffffffffULL : leader;
    out[10] = s.nf(node, NF_ELECTION) & 0xff;
    u32 nt = 0, nv = 0;
    for (u32 k = 0; k < p.mw; k++) {
      nt += (u32)__popc(s.am_word(node, NF_TO_MASK, k));
      nv += (u32)__popc(s.am_word(node, NF_BAL0_AUTHORS, k)) + (u32)__popc(s.am_word(node, NF_BAL1_AUTHORS, k));
    }
    out[11] = nt; out[12] = nv;
    out[13] = s.nf(node, NF_PROPOSED_BLK) ? 1 : 0;
    out[14] = s.nf(node, NF_HTC_ROUND) ? 1 : 0;
  }
  s.store_scalars(s.ld(I_DONE) != 0);
}

#endif  // LBFT_NODE_OPS_H
