// REFERENCE PIN stand-in: the one name main.h / APD.h mention in host declarations.
#ifndef DVP_REF_SHIM_BOOST_FILESYSTEM_HPP_
#define DVP_REF_SHIM_BOOST_FILESYSTEM_HPP_
namespace boost { namespace filesystem { class path {}; } }
#endif
