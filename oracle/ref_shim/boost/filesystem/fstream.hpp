// REFERENCE PIN stand-in: see ../filesystem.hpp
#include <boost/filesystem.hpp>
